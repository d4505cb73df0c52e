// amk_pipeline: several independent control steps in flight on one GPU, behind the C ABI.
//
// A control step of this library (index builds of a fresh depth frame + amk_step_batch) is a chain of dependent launches
// whose dominant kernel is latency-bound: one stream fills ~1/8 of the chip.  Consecutive frames of
// a fleet of robots (or the batches of a sweep) are independent, so the throughput configuration keeps n_slots launches in
// flight, each on its own HIP stream with its own handles -- until round 2 that orchestration lived only in bench.py.
// A slot = {stream, obstacle index, edge index, MPC batch (warm start, workspace), input / output buffers, events}.
// The reference has one robot and one step in flight (AM/src/mpc_obstacle_avoidance_node.cpp:8,
// AvoidanceStateMachine.cpp:322-355); this is the batched counterpart of its per-frame sequence
// FrameKDMap::AddVertex (FrameKDMap.cpp:34-52) -> AvoidanceStateMachine::Step.
//
// Gang (amk_pipeline_config.gang = G > 1): G consecutively submitted frames share ONE set of launches -- the slot's handles
// hold G x n_scenes scenes, frame g occupies scenes [g S, (g + 1) S).  More than ~28 streams collapse on this runtime (32
// hardware queues), so a gang is how MORE scenes are kept in flight than 20-odd slots of one frame hold, in fewer and
// fuller launches: on the bench workload (256-scene frames) 10 slots x 4 frames reach 519 k scene-steps/s in the steady
// state against 466 k for 20 x 1, and 410-422 k against 378 k over a 20-frame burst (same box).
// A frame is only STAGED by submit() until its gang is full; wait() / drain() launch a partly filled gang.
#include "mpc_handle.h"

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <vector>

struct amk_pipeline {
    amk_pipeline_config cfg;
    struct Staged {  // a frame of the open gang
        amk_pipeline_frame frame;           // the caller's record: its DEVICE pointers are read at the launch; its host pointers are copied:
        std::vector<amk_kd *> kf_obstacle, kf_edge;   // frame.kf_*: the caller's keyframe handles behind the slot's own indices (gang 1 only)
        bool has_camera = false;
        amk_frame_camera camera{};          // *frame.camera
        hipEvent_t input_ready = nullptr;   // frame.input_ready: the slot's stream waits for it before reading the inputs
    };
    struct Slot {
        hipStream_t stream = nullptr;
        int queue_mode = AMK_QUEUES_POOLED;   // how `stream` was really created (amk_pipeline_queue_mode)
        std::vector<hipEvent_t> done;   // ring of queue_depth events: done[k % depth] marks the end of the slot's k-th launch
        long long count = 0;            // gang launches issued on this slot
        long long waited = 0;           // launches known to have finished
        amk_kd *obstacle = nullptr, *edge = nullptr;
        amk_mpc *mpc = nullptr;
        amk::DevBuf<double> ref_path, u, x0array, state_quad, pos_x;   // [G S][...]: the gang's contiguous inputs / outputs
        amk::DevBuf<int> flags;
        std::vector<Staged> open;       // frames staged since the last launch (< gang)
        int point_stride = 3;
        // frames that start at the depth image: the slot's own clouds + counts, and mCurFrame.Twc of every scene (persistent)
        amk::DevBuf<float> dcloud, dedge;      // [G S][max_points][3], [G S][max_edge_points][3]
        amk::DevBuf<int> dcount, decount;      // [G S]
        amk::DevBuf<double> Twc;               // [G S][16]
        amk::DevBuf<unsigned char> dwork;      // amk_depth_to_clouds' workspace: the positions of a gang run on one stream, so one serves them
        bool ref_inited[AMK_PIPELINE_MAX_GANG] = {};   // TASK mode: position g holds an mRefPath (a frame with d_ref_path_init ran
                                        // there, and no launch has failed half-way since)
        amk_kfmap *map = nullptr;       // amk_pipeline_config.keyframes.max_frame_count > 0: the slot's keyframe map (gang x n_scenes scenes)
        int fail_status = AMK_OK;       // the slot's newest launch failed half-way with this status: its frames were dropped, their
                                        // results are undefined; reported by that submit() and by wait() / drain() until the next launch
        // the trajectory audit's answers, [G S] each (amk_pipeline_set_path_audit allocates them; never freed before destroy)
        amk::DevBuf<int> audit_stop, audit_leg, audit_src;
        amk::DevBuf<double> audit_t, audit_free;
        amk::DevBuf<float> audit_pts;   // [G S][3]
    };
    int depth = 1, gang = 1;
    std::vector<Slot> slots;
    int next = 0;
    long long submitted = 0;
    int inject_failure = 0;             // tests only (amk__pipeline_inject_failure): the next launch fails at this stage
    int audit_mode = AMK_AUDIT_OFF;     // amk_pipeline_set_path_audit: the stage between the step and the command
    double audit_radius_sq = 0.0;
    int audit_points = 0;               // path points audited: n_legs + 1 <= N
};
extern "C" int amk__pipeline_queue_policy(int pool, int n_slots, int n_classes, int forced, int *mode_out, int *class_out);

namespace {
// The small inputs of the frames of a gang into the slot's contiguous buffers, and their fresh warm starts, in ONE launch
// (as 3 copies + 1 memset per frame they were 16 tiny dispatches in front of every launch of a gang of 4, each of which
// queued behind whatever the other slots were dispatching: 7 % of the summed kernel time with 10 launches in flight).
struct GatherArgs {
    const double *sq[AMK_PIPELINE_MAX_GANG], *px[AMK_PIPELINE_MAX_GANG], *ref[AMK_PIPELINE_MAX_GANG];
    int keep_warm_start[AMK_PIPELINE_MAX_GANG];
    double *sq_dst, *px_dst, *ref_dst, *w0;   // [G][n_*]; sq_dst / px_dst NULL: not copied (gang 1 reads the caller's)
    int n_sq, n_px, n_ref, n_w0;              // doubles per frame
};
__global__ __launch_bounds__(256) void pipeline_gather_kernel(const GatherArgs a) {
    const int g = blockIdx.y;
    const int stride = gridDim.x * 256, t0 = blockIdx.x * 256 + threadIdx.x;
    if (a.sq_dst && a.sq[g]) {
        for (int i = t0; i < a.n_sq; i += stride) a.sq_dst[(size_t)g * a.n_sq + i] = a.sq[g][i];
        for (int i = t0; i < a.n_px; i += stride) a.px_dst[(size_t)g * a.n_px + i] = a.px[g][i];
    }
    if (a.ref[g])   // (a TASK-mode frame's path is the prologue kernel's business)
        for (int i = t0; i < a.n_ref; i += stride) a.ref_dst[(size_t)g * a.n_ref + i] = a.ref[g][i];
    if (!a.keep_warm_start[g])
        for (int i = t0; i < a.n_w0; i += stride) a.w0[(size_t)g * a.n_w0 + i] = 0.0;
}
// ... and the controls of every frame to where its caller wants them; for TASK-mode frames also what the node publishes:
// PubCmd(u) when isSafety, else PubSlowDownCmd (AvoidanceStateMachine.cpp:345-350,369-397)
struct ScatterArgs {
    double *dst[AMK_PIPELINE_MAX_GANG];   // NULL: stays in the slot's buffer only
    double *cmd[AMK_PIPELINE_MAX_GANG];   // NULL: no command wanted
    const double *odom[AMK_PIPELINE_MAX_GANG];
    const double *u;
    const int *flags;
    int n_u, S;
    double kp, kd, a_max_xy, a_max_z;
};
__global__ __launch_bounds__(256) void pipeline_scatter_kernel(const ScatterArgs a) {
#pragma clang fp contract(off)   // the command is compared bit for bit with the host twin (avoid_mpc_amd/flight.py: command)
    const int g = blockIdx.y;
    if (a.dst[g] && a.dst[g] != a.u + (size_t)g * a.n_u)
        for (int i = blockIdx.x * 256 + threadIdx.x; i < a.n_u; i += gridDim.x * 256) a.dst[g][i] = a.u[(size_t)g * a.n_u + i];
    if (a.cmd[g]) {
        for (int i = blockIdx.x * 256 + threadIdx.x; i < a.S * 3; i += gridDim.x * 256) {
            const int s = i / 3, c = i - 3 * s;
            const size_t gs = (size_t)g * a.S + s;
            double v;
            if (a.flags[gs * 4 + 0]) v = a.u[gs * 4 + c];                                  // PubCmd :369-378
            else {                                                                         // PubSlowDownCmd :379-397
                const double *o = a.odom[g] + (size_t)s * 10;
                v = -o[4 + c] * a.kp - o[7 + c] * a.kd + (c == 2 ? 9.8 : 0.0);
                const double lim = c == 2 ? a.a_max_z : a.a_max_xy;
                v = fmax(-lim, fmin(lim, v));
            }
            a.cmd[g][i] = v;
        }
    }
}
// AMK_AUDIT_SLOW_DOWN, behind pipeline_scatter_kernel and only then: a scene that the step called safe (flags[0] == 1) but whose
// audited trajectory stops gets PubSlowDownCmd after all -- the else-branch above, the same expression.  Nothing else is written.
struct VetoArgs {
    double *cmd[AMK_PIPELINE_MAX_GANG];   // NULL: not a TASK frame, or no command wanted
    const double *odom[AMK_PIPELINE_MAX_GANG];
    const int *flags, *stop;
    int S;
    double kp, kd, a_max_xy, a_max_z;
};
__global__ __launch_bounds__(256) void pipeline_audit_veto_kernel(const VetoArgs a) {
#pragma clang fp contract(off)   // the command is compared bit for bit with the host twin (avoid_mpc_amd/flight.py: command)
    const int g = blockIdx.y;
    if (!a.cmd[g]) return;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < a.S * 3; i += gridDim.x * 256) {
        const int s = i / 3, c = i - 3 * s;
        const size_t gs = (size_t)g * a.S + s;
        if (!a.flags[gs * 4 + 0] || !a.stop[gs]) continue;   // (not safe: the slow-down command is there already; safe and free: u stays)
        const double *o = a.odom[g] + (size_t)s * 10;
        double v = -o[4 + c] * a.kp - o[7 + c] * a.kd + (c == 2 ? 9.8 : 0.0);
        const double lim = c == 2 ? a.a_max_z : a.a_max_xy;
        v = fmax(-lim, fmin(lim, v));
        a.cmd[g][i] = v;
    }
}

// mCurFrame.Twc = mat4Twb * mParamTbc (FrameKDMap.cpp:50) for the scenes whose frame produced an obstacle cloud (:39-41 returns
// before it otherwise); Twc == nullptr-initialised slots start from the identity (pipeline_twc_init_kernel)
__global__ __launch_bounds__(256) void pipeline_twc_update_kernel(const double *__restrict__ Twb, const int *__restrict__ counts,
                                                                  double *__restrict__ Twc, int S, const amk_depth_params prm) {
#pragma clang fp contract(off)   // the product the host twin forms (include/avoid_mpc_amd/frame_kd_map.hpp: AddVertex), sum in k order
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= S * 16) return;
    const int s = e / 16, i = (e % 16) / 4, j = e % 4;
    if (counts[s] == 0) return;
    double acc = 0.0;
    for (int k = 0; k < 4; ++k) acc += Twb[s * 16 + 4 * i + k] * prm.Tbc[4 * k + j];
    Twc[e] = acc;
}
__global__ __launch_bounds__(256) void pipeline_twc_init_kernel(double *__restrict__ Twc, int n) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n * 16) Twc[e] = (e % 16) % 5 == 0 ? 1.0 : 0.0;
}

// TASK-mode prologue (AvoidanceStateMachine.cpp:24-54,183-203,322-330): one wavefront per scene runs GetInitPath on the slot's
// own mRefPath (optionally re-initialised from the caller's first) and GetCurStateQuad for every re-plan pass.
struct PrologueArgs {
    const double *odom[AMK_PIPELINE_MAX_GANG];       // NULL: not a TASK-mode frame
    const double *ref_init[AMK_PIPELINE_MAX_GANG];   // NULL: the slot's own path
    double age[AMK_PIPELINE_MAX_GANG];
    const double *goal[AMK_PIPELINE_MAX_GANG];       // [S][3] or NULL: mStateGlobalGoal (task global_goal)
    double *sq_dst, *px_dst, *ref_dst;               // [G][S][mi][10], [G][S], [G][S][N][10]
    int S, N, mi;
    double decay, iter_time, farest, height, speed, T, dt;
    int use_odom_est, task;
};
__global__ __launch_bounds__(256) void pipeline_task_prologue_kernel(const PrologueArgs a) {
#pragma clang fp contract(off)   // bit-identical to the host twins (avoid_mpc_amd/fsm.py, include/avoid_mpc_amd/avoidance_step.hpp)
    const int g = blockIdx.y;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const bool live = a.odom[g] && s < a.S;
    const size_t gs = (size_t)g * a.S + (live ? s : 0);
    const double *o = live ? a.odom[g] + (size_t)s * 10 : nullptr;
    double *ref = a.ref_dst + gs * a.N * 10;
    const double *src = (live && a.ref_init[g]) ? a.ref_init[g] + (size_t)s * a.N * 10 : ref;
    // GetInitPath: mRefPath[i] = mRefPath[i + 1] with z = height, i < N - 1; the last point is the goal.  Every element is read
    // before any is written (the shift runs in place).
    const int n_shift = (a.N - 1) * 10;
    double v[5];   // N <= AMK_MAX_HORIZON = 32: 310 elements <= 5 x 64
    for (int k = 0; k < 5; ++k) {
        const int e = k * 64 + lane;
        v[k] = (live && e < n_shift) ? src[e + 10] : 0.0;
    }
    // the goal (:26-45), from the path as it is BEFORE the shift.  forward: speed * T ahead of the odometry position, capped;
    // global_goal: from the path's last point towards mStateGlobalGoal by at most speed * dt (dPos.normalized() * min(|dPos|, .):
    // Eigen's normalized() divides by the norm when it is positive and returns the vector unchanged otherwise)
    double goalx = 0.0, goaly = 0.0, goalz = a.height;
    if (live) {
        if (a.task == AMK_TASK_GLOBAL_GOAL) {
            const double *gg = a.goal[g] ? a.goal[g] + (size_t)s * 3 : nullptr;
            const double g0 = gg ? gg[0] : 0.0, g1 = gg ? gg[1] : 0.0, g2 = gg ? gg[2] : a.height;
            const double *last = src + n_shift;
            const double d0 = g0 - last[0], d1 = g1 - last[1], d2 = g2 - last[2];
            const double z = (d0 * d0 + d1 * d1) + d2 * d2, nrm = sqrt(z);
            const double step = fmin(nrm, a.speed * a.dt);
            const double e0 = z > 0.0 ? d0 / nrm : d0, e1 = z > 0.0 ? d1 / nrm : d1, e2 = z > 0.0 ? d2 / nrm : d2;
            goalx = last[0] + e0 * step; goaly = last[1] + e1 * step; goalz = last[2] + e2 * step;
        } else {
            goalx = fmin(a.speed * a.T + o[0], a.farest);
        }
    }
    __syncthreads();
    if (live) {
        for (int k = 0; k < 5; ++k) {
            const int e = k * 64 + lane;
            if (e < n_shift) ref[e] = (e % 10 == 2) ? goalz : v[k];
        }
        if (lane < 10) ref[n_shift + lane] = lane == 0 ? goalx : (lane == 1 ? goaly : (lane == 2 ? goalz : (lane == 4 ? a.speed : 0.0)));
        // GetCurStateQuad(start_i + decay_i) (:329-330,343): pass 0 extrapolates by odom_age + decay; pass i >= 1 starts i passes
        // later and extrapolates by the MEASURED duration of pass i - 1 -- with the clock model "every pass takes iter_time":
        // odom_age + (i + 1) * iter_time (written iter_time + i * iter_time so that the default iter_time = decay
        // keeps the bits of rounds 3-4)
        for (int e = lane; e < a.mi * 10; e += 64) {
            const int i = e / 10, j = e - 10 * i;
            const double dt = a.age[g] + (i == 0 ? a.decay : a.iter_time) + i * a.iter_time;
            double r;
            if (j < 3) r = a.use_odom_est ? o[j] + o[4 + j] * dt + 0.5 * o[7 + j] * dt * dt : o[j];
            else if (j == 3) r = o[3];
            else if (j < 7) r = a.use_odom_est ? o[j] + o[j + 3] * dt : o[j];
            else r = o[j];
            a.sq_dst[(gs * a.mi + i) * 10 + j] = r;
        }
        if (lane == 0) a.px_dst[gs] = o[0];   // mPos.x() of GetRefStates (:251): the odometry position, not the extrapolated one
    }
}

using Slot = amk_pipeline::Slot;
bool env_flag(const char *name) { const char *e = std::getenv(name); return e && e[0] == '1'; }
// Host microseconds for the diagnostics of AMK_PIPELINE_TRACE=1.  With the trace off no clock is read.
struct Stopwatch {
    static bool on() { static const bool trace = env_flag("AMK_PIPELINE_TRACE"); return trace; }
    static double now() { return on() ? std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count() : 0.0; }
    double t0 = now(), us[3] = {};   // us: the laps taken so far, by number (launch_gang's trace line prints three)
    double lap(int i = 0) { const double t = now(); us[i] = t - t0; t0 = t; return us[i]; }   // since the start or the last lap
};
// DevBuf::alloc for a list of (buffer, count) pairs, in order; the first error ends it
inline hipError_t alloc_all() { return hipSuccess; }
template <typename T, typename... Rest>
hipError_t alloc_all(amk::DevBuf<T> &buf, size_t count, Rest &&...rest) {
    const hipError_t e = buf.alloc(count);
    return e != hipSuccess ? e : alloc_all(rest...);
}
Slot *slot_at(amk_pipeline *p, int slot) { return (p && slot >= 0 && slot < (int)p->slots.size()) ? &p->slots[slot] : nullptr; }
Slot *slot_of(amk_pipeline *p, int ticket) {   // ticket = position in the gang * n_slots + slot
    return (p && ticket >= 0 && ticket < (int)p->slots.size() * p->gang) ? &p->slots[ticket % (int)p->slots.size()] : nullptr;
}
// Waits for a slot's launch.  hipEventSynchronize parks the thread on an HSA signal; with AMK_PIPELINE_SPIN=1 the thread polls
// hipEventQuery instead (diagnostics: tools/experiments/rccl_presence.py).
int wait_event(hipEvent_t ev) {
    static const bool spin = env_flag("AMK_PIPELINE_SPIN");
    if (!spin) {
        AMK_HIP(hipEventSynchronize(ev));
        return AMK_OK;
    }
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return AMK_OK;
        if (e != hipErrorNotReady) return amk::hip_fail(e);
    }
}
// One launch of a slot's open gang: what its stages share.  Position g occupies scenes [g S, (g + 1) S) of the slot's handles.
struct Launch {
    amk_pipeline *p;
    const amk_pipeline_config &c;   // p->cfg
    Slot &s;
    int G, S, N, mi, filled;   // filled < G: wait / drain before the G-th submit; the launch runs on the leading scenes only
    hipStream_t st;
    // per position, written once by the stage that decides them (depth_stage): the clouds and counts the indices are built from,
    // the counts whose zeros keep a scene's previous frame (a depth frame's; else null), mCurFrame.Twc for the slot's map
    const float *cl[AMK_PIPELINE_MAX_GANG], *ed[AMK_PIPELINE_MAX_GANG];
    const int *cc[AMK_PIPELINE_MAX_GANG], *ec[AMK_PIPELINE_MAX_GANG], *keep[AMK_PIPELINE_MAX_GANG];
    const double *twc[AMK_PIPELINE_MAX_GANG];
    bool any_task, any_depth, own_inputs;   // own_inputs: the step reads the slot's contiguous copies (gang 1 without TASK mode: the caller's)
    const amk_pipeline_frame &frame(int g) const { return s.open[g].frame; }
    int wait_for_inputs(), restart_robots(), gather_inputs(), depth_stage();   // the stages, in launch_gang's order
    int build_indices(Stopwatch &watch), control_step(), path_audit(), finish();
    int ensure_depth_buffers(long long work_bytes), depth_camera(amk_frame_camera *cam);   // (parts of depth_stage and control_step)
};
int Launch::wait_for_inputs() {   // inputs produced on the caller's streams: ordered on the device, not by the host
    for (const auto &o : s.open)
        if (o.input_ready) AMK_HIP(hipStreamWaitEvent(st, o.input_ready, 0));
    return AMK_OK;
}
// A robot that starts over (a TASK frame with d_ref_path_init: InitCircleState's role) also starts with a new FrameKDMap:
// no keyframes, mCurFrame.Twc = identity -- before the depth stage, whose edge cloud goes through that (stale) pose (:209).
// (Without a map the slot's Twc keeps its round-4 behaviour: it persists.)
int Launch::restart_robots() {
    if (!s.map) return AMK_OK;
    for (int g = 0; g < filled; ++g) {
        if (!(frame(g).d_odom && frame(g).d_ref_path_init)) continue;
        if (const int rr = amk_kfmap_reset(s.map, g * S, S, st); rr != AMK_OK) return rr;
        if (!s.Twc.p) continue;
        hipLaunchKernelGGL(pipeline_twc_init_kernel, dim3((S * 16 + 255) / 256), dim3(256), 0, st, s.Twc.p + (size_t)g * S * 16, S);
        AMK_HIP(hipGetLastError());
    }
    return AMK_OK;
}
// The small inputs into the slot's buffers (pipeline_gather_kernel), then the TASK frames' prologue
int Launch::gather_inputs() {
    GatherArgs ga{};
    PrologueArgs pa{};
    for (int g = 0; g < filled; ++g) {
        const amk_pipeline_frame &f = frame(g);
        const bool task = f.d_odom != nullptr;
        any_task = any_task || task;
        ga.sq[g] = task ? nullptr : f.d_state_quad; ga.px[g] = task ? nullptr : f.d_pos_x; ga.ref[g] = task ? nullptr : f.d_ref_path_init;
        pa.odom[g] = f.d_odom; pa.ref_init[g] = f.d_ref_path_init; pa.age[g] = f.odom_age; pa.goal[g] = f.d_global_goal;
        // fresh frame: mRefPath after GetInitPath, zero warm start unless the caller carries it over (HighLvlMpc.cpp:26-27,35,129)
        ga.keep_warm_start[g] = f.keep_warm_start;
    }
    own_inputs = G > 1 || any_task;
    ga.sq_dst = own_inputs ? s.state_quad.p : nullptr; ga.px_dst = own_inputs ? s.pos_x.p : nullptr;
    ga.ref_dst = s.ref_path.p; ga.w0 = s.mpc->w0.p;
    ga.n_sq = S * mi * 10; ga.n_px = S; ga.n_ref = S * N * 10; ga.n_w0 = S * s.mpc->nx;
    const int longest = ga.n_w0 > ga.n_ref ? ga.n_w0 : ga.n_ref;
    int bx = (longest + 1023) / 1024;
    bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
    hipLaunchKernelGGL(pipeline_gather_kernel, dim3(bx, filled), dim3(256), 0, st, ga);
    AMK_HIP(hipGetLastError());
    if (!any_task) return AMK_OK;
    const amk_task_params &t = c.task;
    pa.sq_dst = s.state_quad.p; pa.px_dst = s.pos_x.p; pa.ref_dst = s.ref_path.p;
    pa.S = S; pa.N = N; pa.mi = mi;
    pa.decay = t.decay; pa.iter_time = t.iter_time > 0 ? t.iter_time : t.decay; pa.farest = t.farest_point; pa.height = t.height;
    pa.speed = c.step.speed; pa.T = c.T; pa.dt = c.dt; pa.use_odom_est = t.use_odom_est; pa.task = t.task;
    hipLaunchKernelGGL(pipeline_task_prologue_kernel, dim3((S + 3) / 4, filled), dim3(256), 0, st, pa);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}
// The slot's own clouds, counts and Twc, allocated by its first depth frame -- or again after an attempt that ran out of memory
// half-way: all six buffers or none.  Every scene's Twc starts from the identity.  The workspace of amk_depth_to_clouds
// is the only one that depends on the image: a later frame with more rows gets a larger one (hipFree waits for the device, so no
// launch in flight still reads the old one; the other five, and with them every scene's Twc, stay).
int Launch::ensure_depth_buffers(long long work_bytes) {
    const auto release_all = [this] { s.dcloud.release(); s.dedge.release(); s.dcount.release(); s.decount.release(); s.Twc.release(); s.dwork.release(); };
    if (s.dcloud.p && s.dedge.p && s.dcount.p && s.decount.p && s.Twc.p && s.dwork.p) {
        if ((long long)s.dwork.n >= work_bytes) return AMK_OK;
        if (const hipError_t e = s.dwork.alloc((size_t)work_bytes); e != hipSuccess) {
            release_all();
            return amk::hip_fail(e);
        }
        return AMK_OK;
    }
    const size_t GS = (size_t)G * S;
    const hipError_t e = alloc_all(s.dcloud, GS * c.max_points * 3, s.dedge, GS * c.max_edge_points * 3, s.dcount, GS, s.decount, GS, s.Twc, GS * 16,
                                   s.dwork, (size_t)work_bytes);
    if (e != hipSuccess) {
        release_all();
        return amk::hip_fail(e);
    }
    hipLaunchKernelGGL(pipeline_twc_init_kernel, dim3((unsigned)((GS * 16 + 255) / 256)), dim3(256), 0, st, s.Twc.p, (int)GS);
    AMK_HIP(hipGetLastError());
    return AMK_OK;
}
// Where every position's index is built from: the caller's clouds, or -- a frame that starts at the depth image -- ProcessDepth +
// BuildEdgeCloud (FrameKDMap.cpp:90-130,176-214) into the slot's own, and the new mCurFrame.Twc behind them
int Launch::depth_stage() {
    for (int g = 0; g < filled; ++g) {
        const amk_pipeline_frame &f = frame(g);
        if (!f.d_depth) {
            cl[g] = f.d_cloud; ed[g] = f.d_edge; cc[g] = f.d_cloud_counts; ec[g] = f.d_edge_counts; keep[g] = nullptr; twc[g] = f.d_Twc_cur;
            continue;
        }
        if (s.point_stride != 3) return AMK_ERR_INVALID_ARG;   // the slot's own clouds are packed xyz
        long long work_bytes = 0;
        if (const int rc = amk_depth_clouds_work_bytes(f.depth_rows, f.depth_cols, c.depth.resize_scale, S, &work_bytes); rc != AMK_OK) return rc;
        if (const int rc = ensure_depth_buffers(work_bytes); rc != AMK_OK) return rc;
        any_depth = true;
        const size_t o = (size_t)g * S;
        float *dc = s.dcloud.p + o * c.max_points * 3, *de = s.dedge.p + o * c.max_edge_points * 3;
        const long long img = (long long)f.depth_rows * f.depth_cols;
        const int rc = amk_depth_to_clouds(f.d_depth, f.depth_type, f.depth_rows, f.depth_cols, img, S, &c.depth, f.d_Twb, s.Twc.p + o * 16, dc,
                                           (long long)c.max_points * 3, s.dcount.p + o, de, (long long)c.max_edge_points * 3, s.decount.p + o, 3,
                                           s.dwork.p, (long long)s.dwork.n, st);
        if (rc != AMK_OK) return rc;
        hipLaunchKernelGGL(pipeline_twc_update_kernel, dim3((S * 16 + 255) / 256), dim3(256), 0, st, f.d_Twb, s.dcount.p + o, s.Twc.p + o * 16, S, c.depth);
        AMK_HIP(hipGetLastError());
        cl[g] = dc; ed[g] = de; cc[g] = keep[g] = s.dcount.p + o; ec[g] = s.decount.p + o; twc[g] = s.Twc.p + o * 16;
    }
    return AMK_OK;
}
// FrameKDMap::AddVertex: obstacle index and edge index of every frame (FrameKDMap.cpp:44-47)
int Launch::build_indices(Stopwatch &watch) {
    if (!s.map) {
        if (G == 1 && !any_depth) return amk_kd_build_pair(s.obstacle, cl[0], cc[0], s.edge, ed[0], ec[0], s.point_stride, st);
        return amk::kd_build_gang(s.obstacle, s.edge, filled, S, cl, cc, ed, ec, s.point_stride, st, any_depth ? keep : nullptr);
    }
    // ... into the slot's keyframe map: the scenes' own physical slots, mCurFrame.Twc, then KeyframeThreadWorker's body
    for (int g = 0; g < filled; ++g)
        if (!twc[g]) return AMK_ERR_INVALID_ARG;   // (submit() checked)
    // AddVertex of every position of the gang: one bookkeeping launch + one build launch (both trees of all frames)
    int rc = amk::kfmap_add_vertex_gang(s.map, filled, S, cl, cc, ed, ec, s.point_stride, twc, st);
    if (rc != AMK_OK) return rc;
    watch.lap(0);
    rc = amk_kfmap_update(s.map, st);
    watch.lap(1);
    return rc;
}
// The camera model of the step over the slot's map (ONE per launch, position 0's: submit() makes a gang agree on it): a cloud
// frame brings it; a depth frame's is the FrameKDMap constructor's down-scaled intrinsics and ProcessDepth's image size (:21-24,106-107)
int Launch::depth_camera(amk_frame_camera *cam) {
    const amk_pipeline_frame &f = frame(0);
    const amk_depth_params &d = c.depth;
    cam->fx = d.fx / d.resize_scale; cam->fy = d.fy / d.resize_scale; cam->cx = d.cx / d.resize_scale; cam->cy = d.cy / d.resize_scale;
    cam->depth_max = d.depth_max;
    return amk_depth_out_size(f.depth_rows, f.depth_cols, d.resize_scale, &cam->width, &cam->height);
}
// One control step over all frames: over the slot's map, over [this frame, the caller's keyframes ...], or over this frame alone
int Launch::control_step() {
    const amk_pipeline::Staged &o = s.open[0];
    double *u = (G == 1 && o.frame.d_u_out && !any_task) ? o.frame.d_u_out : s.u.p;
    const double *sq = own_inputs ? s.state_quad.p : o.frame.d_state_quad, *px = own_inputs ? s.pos_x.p : o.frame.d_pos_x;
    const amk::RunScenes leading(s.mpc, filled * S);   // (a gang that is not full; reset on every way out)
    if (s.map) {   // mVecQueryVector = [current, keyframes but the newest] of every scene
        amk_frame_camera cam = o.camera;
        if (const int rc = o.frame.d_depth ? depth_camera(&cam) : AMK_OK; rc != AMK_OK) return rc;
        return amk_kfmap_step(s.map, (o.has_camera || o.frame.d_depth) ? &cam : nullptr, s.mpc, &c.step, sq, px, s.ref_path.p, u, s.x0array.p, s.flags.p, st);
    }
    if (o.kf_obstacle.empty()) return amk_step_batch(s.obstacle, s.edge, s.mpc, &c.step, sq, px, s.ref_path.p, u, s.x0array.p, s.flags.p, st);
    // mVecQueryVector = [this frame, keyframes ...] (gang 1: submit() checked)
    std::vector<amk_kd *> kd_ob{s.obstacle}, kd_ed{s.edge};
    kd_ob.insert(kd_ob.end(), o.kf_obstacle.begin(), o.kf_obstacle.end());
    kd_ed.insert(kd_ed.end(), o.kf_edge.begin(), o.kf_edge.end());
    const double *twc_cur = o.frame.d_Twc_cur ? o.frame.d_Twc_cur : (o.frame.d_depth ? s.Twc.p : nullptr);
    return amk_step_batch_frames(kd_ob.data(), kd_ed.data(), (int)kd_ob.size(), twc_cur, o.has_camera ? &o.camera : nullptr, s.mpc, &c.step, sq, px,
                                 s.ref_path.p, u, s.x0array.p, s.flags.p, st);
}
// The trajectory audit (amk_pipeline_set_path_audit; launch_gang calls it only when the mode is not OFF): the path cast on the
// step's own x0array -- a scene's path is its first audit_points rows of 14, row 0 = X0 -- over the filled * S leading scenes,
// against the slot's map as it stands after this period's AddVertex and update, else against its obstacle index
int Launch::path_audit() {
    const amk::PathCastOut out{s.audit_stop.p, s.audit_leg.p, s.audit_t.p, s.audit_free.p, s.audit_pts.p, s.audit_src.p};
    if (s.map)
        return amk::kfmap_path_cast_scenes(s.map, filled * S, s.x0array.p, 14, (long long)N * 14, p->audit_points, p->audit_radius_sq, 0, out, st);
    return amk::kd_path_cast_scenes(s.obstacle, filled * S, s.x0array.p, 14, (long long)N * 14, p->audit_points, p->audit_radius_sq, out, st);
}
// The controls to where the callers want them (pipeline_scatter_kernel), the completion event, the slot's books
int Launch::finish() {
    if (own_inputs) {
        ScatterArgs sa{};
        bool any = false;
        for (int g = 0; g < filled; ++g) {
            const amk_pipeline_frame &f = frame(g);
            sa.dst[g] = f.d_u_out; sa.cmd[g] = f.d_odom ? f.d_cmd_out : nullptr; sa.odom[g] = f.d_odom;
            any = any || sa.dst[g] || sa.cmd[g];
        }
        sa.u = s.u.p; sa.flags = s.flags.p; sa.n_u = S * 4; sa.S = S;
        sa.kp = c.task.slow_down_kp; sa.kd = c.task.slow_down_kd; sa.a_max_xy = c.task.a_max_xy; sa.a_max_z = c.task.a_max_z;
        if (any) {
            hipLaunchKernelGGL(pipeline_scatter_kernel, dim3((sa.n_u + 255) / 256 > 16 ? 16 : (sa.n_u + 255) / 256, filled), dim3(256), 0, st, sa);
            AMK_HIP(hipGetLastError());
        }
        if (p->audit_mode == AMK_AUDIT_SLOW_DOWN) {   // the veto, behind the command it overrides
            VetoArgs va{};
            bool any_cmd = false;
            for (int g = 0; g < filled; ++g) {
                va.cmd[g] = sa.cmd[g]; va.odom[g] = sa.odom[g];
                any_cmd = any_cmd || va.cmd[g];
            }
            va.flags = s.flags.p; va.stop = s.audit_stop.p; va.S = S;
            va.kp = sa.kp; va.kd = sa.kd; va.a_max_xy = sa.a_max_xy; va.a_max_z = sa.a_max_z;
            if (any_cmd) {
                hipLaunchKernelGGL(pipeline_audit_veto_kernel, dim3((S * 3 + 255) / 256 > 16 ? 16 : (S * 3 + 255) / 256, filled), dim3(256), 0, st, va);
                AMK_HIP(hipGetLastError());
            }
        }
    }
    AMK_HIP(hipEventRecord(s.done[s.count % p->depth], st));
    ++s.count;
    for (int g = 0; g < filled; ++g)
        if (frame(g).d_odom && frame(g).d_ref_path_init) s.ref_inited[g] = true;
    s.open.clear();
    return AMK_OK;
}
// Launches the slot's open gang (not empty): both index builds of every staged frame in one launch, one control step over all of
// them.  A stage that fails ends the launch; what the stages before it enqueued stays enqueued (launch_slot).
int launch_gang(amk_pipeline *p, Slot &s) {
    const int filled = (int)s.open.size();
    if (filled > p->gang || filled > AMK_PIPELINE_MAX_GANG) return AMK_ERR_INVALID_ARG;   // (submit() never stages more than a gang)
    // AMK_TIES_AUTO on the slot's handles (amk_pipeline_kd) is for the single-frame step only (header): refused before anything is launched
    if ((s.map || !s.open[0].kf_obstacle.empty()) && ((s.obstacle && s.obstacle->tie_order == AMK_TIES_AUTO) || (s.edge && s.edge->tie_order == AMK_TIES_AUTO)))
        return AMK_ERR_UNSUPPORTED;
    Launch L{p, p->cfg, s, p->gang, p->cfg.n_scenes, amk_mpc_horizon(s.mpc), p->cfg.step.mpc_max_iter, filled, s.stream};
    int rc;
    if ((rc = L.wait_for_inputs()) != AMK_OK) return rc;
    if ((rc = L.restart_robots()) != AMK_OK) return rc;
    if ((rc = L.gather_inputs()) != AMK_OK) return rc;
    if (p->inject_failure == 1) { p->inject_failure = 0; return AMK_ERR_HIP; }
    if ((rc = L.depth_stage()) != AMK_OK) return rc;
    Stopwatch watch;   // AMK_PIPELINE_TRACE=1: host microseconds spent enqueueing the build and the step
    if ((rc = L.build_indices(watch)) != AMK_OK) return rc;
    if (p->inject_failure == 2) { p->inject_failure = 0; return AMK_ERR_HIP; }
    rc = L.control_step();
    if (Stopwatch::on())
        fprintf(stderr, "amk_pipeline launch: add_vertex %.0f us, map update %.0f us, step %.0f us (host enqueue time)\n", watch.us[0],
                watch.us[1], watch.lap(2));
    if (rc != AMK_OK) return rc;
    if (p->audit_mode != AMK_AUDIT_OFF && (rc = L.path_audit()) != AMK_OK) return rc;
    return L.finish();
}
// launch_gang, if a gang is open, with the slot left consistent whatever happens: on a failure half-way (a build or a step that
// could not be launched) the staged frames are DROPPED -- a later submit() starts a new gang instead of re-launching a
// half-consumed one, and wait() / drain() have an event to wait for (what did get enqueued stays ordered on the slot's stream)
// and report the failure.  The round robin moves on either way.
int launch_slot(amk_pipeline *p, Slot &s) {
    if (s.open.empty()) return AMK_OK;
    Stopwatch watch;
    const int st = launch_gang(p, s);
    if (Stopwatch::on()) fprintf(stderr, "amk_pipeline launch_gang total: %.0f us (host)\n", watch.lap());
    if (st != AMK_OK) {
        // What had been enqueued before the failure stays enqueued: a TASK frame's GetInitPath may already have shifted the slot's
        // mRefPath, its warm start may have been reset, a depth frame's Twc may have moved on.  The slot's persistent
        // TASK state is therefore declared lost: the next TASK frame at any position of this slot must bring d_ref_path_init
        // (submit() rejects it otherwise) -- re-submitting the failed period as it was would shift the path twice.
        for (bool &b : s.ref_inited) b = false;
        s.open.clear();
        (void)hipEventRecord(s.done[s.count % p->depth], s.stream);
        ++s.count;
    }
    s.fail_status = st;
    if (&s == &p->slots[p->next]) p->next = (p->next + 1) % (int)p->slots.size();
    return st;
}
// Hardware queues.  The runtime multiplexes a process's streams onto a pool of GPU_MAX_HW_QUEUES hardware queues (4 unless the
// host exported more before its first HIP call), and two streams on one queue serialise: 10 slots on 4 queues keep 4 chains in
// flight, not 10.  The runtime keeps one such pool per stream priority class, so a pipeline whose slots
// are spread over the classes obtains a queue per slot without the host's help -- amk__pipeline_queue_policy says how, per slot.
// (A stream with a CU mask, hipExtStreamCreateWithCUMask, also gets a queue outside the pool, but it is a BLOCKING stream: it
// synchronises with the null stream, which a pipeline's slots must not -- profiles/pipeline_queues_ab.txt section 2.)
int env_int(const char *name, int absent) {
    const char *e = std::getenv(name);
    const int v = e ? std::atoi(e) : 0;
    return v > 0 ? v : absent;
}
int forced_queue_mode() {   // AMK_PIPELINE_QUEUES=pooled|priority (A/B runs, tests); anything else: automatic (-1)
    const char *e = std::getenv("AMK_PIPELINE_QUEUES");
    if (!e) return -1;
    return !std::strcmp(e, "pooled") ? AMK_QUEUES_POOLED : !std::strcmp(e, "priority") ? AMK_QUEUES_PRIORITY : -1;
}
int g_fail_queue_creation = 0;   // tests only (amk__pipeline_inject_failure(NULL, 3)): the next create's priority stream calls fail
// The slot's stream in the mode the policy gave it; a creation call that fails leaves the slot with a pooled stream.
int create_stream(Slot &s, int mode, int priority, bool fail) {
    s.stream = nullptr;
    s.queue_mode = AMK_QUEUES_POOLED;
    if (mode == AMK_QUEUES_PRIORITY) {
        if (!fail && hipStreamCreateWithPriority(&s.stream, hipStreamNonBlocking, priority) == hipSuccess) {
            s.queue_mode = AMK_QUEUES_PRIORITY;
            return AMK_OK;
        }
        (void)hipGetLastError();   // (the failed call's sticky record)
        s.stream = nullptr;
    }
    AMK_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    return AMK_OK;
}
// A slot's stream, events, handles and buffers; what a failure leaves behind is amk_pipeline_destroy's
int create_slot(const amk_pipeline *p, Slot &s, int queue_mode, int priority, bool fail_queue) {
    const amk_pipeline_config &cfg = p->cfg;
    const int GS = p->gang * cfg.n_scenes;
    if (const int st = create_stream(s, queue_mode, priority, fail_queue); st != AMK_OK) return st;
    s.done.assign(p->depth, nullptr);
    for (auto &ev : s.done) AMK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    int st;
    if ((st = amk_kd_create(GS, cfg.max_points, &s.obstacle)) != AMK_OK) return st;
    if ((st = amk_kd_create(GS, cfg.max_edge_points, &s.edge)) != AMK_OK) return st;
    if ((st = amk_mpc_create(cfg.T, cfg.dt, cfg.nearest_point_num, GS, &s.mpc)) != AMK_OK) return st;
    if (cfg.keyframes.max_frame_count > 0) {
        amk_kfmap_params kp = cfg.keyframes;
        auto all_zero = [](const double *T) { bool z = true; for (int e = 0; e < 16; ++e) z = z && T[e] == 0.0; return z; };
        // mParamTbc: the map's own field when it is set, else the depth configuration's (one extrinsic serves both in the
        // reference, FrameKDMap.cpp:15), else camera frame = body frame
        if (all_zero(kp.Tbc)) std::memcpy(kp.Tbc, cfg.depth.Tbc, sizeof kp.Tbc);
        if (all_zero(kp.Tbc)) kp.Tbc[0] = kp.Tbc[5] = kp.Tbc[10] = kp.Tbc[15] = 1.0;
        if ((st = amk_kfmap_create(GS, cfg.max_points, cfg.max_edge_points, &kp, &s.map)) != AMK_OK) return st;
    }
    const size_t S = GS, N = amk_mpc_horizon(s.mpc);
    AMK_HIP(alloc_all(s.ref_path, S * N * 10, s.u, S * 4, s.x0array, S * N * 14, s.flags, S * 4, s.state_quad, S * cfg.step.mpc_max_iter * 10, s.pos_x, S));
    return AMK_OK;
}
// submit()'s first refusals: what is wrong with a frame's own arguments, whichever slot it goes to
int frame_args(const amk_pipeline_config &c, const amk_pipeline_frame *f) {
    if (f->d_depth) {   // a frame that starts at the depth image
        if (!f->d_Twb || f->depth_rows <= 0 || f->depth_cols <= 0 || (f->depth_type != AMK_DEPTH_U16 && f->depth_type != AMK_DEPTH_F32))
            return AMK_ERR_INVALID_ARG;
        int w = 0, h = 0;
        if (amk_depth_out_size(f->depth_rows, f->depth_cols, c.depth.resize_scale, &w, &h) != AMK_OK) return AMK_ERR_INVALID_ARG;
        if ((long long)w * h > c.max_points || (long long)w * h > c.max_edge_points) return AMK_ERR_INVALID_ARG;
        if (w > AMK_DEPTH_MAX_WIDTH) return AMK_ERR_UNSUPPORTED;   // (amk_depth_to_clouds: any number of pixels, bands of whole rows)
    } else if (!f->d_cloud || !f->d_edge) return AMK_ERR_INVALID_ARG;
    if (!f->d_odom && (!f->d_state_quad || !f->d_pos_x || !f->d_ref_path_init)) return AMK_ERR_INVALID_ARG;
    return (f->n_keyframes < 0 || f->n_keyframes > AMK_MAX_FRAMES - 1) ? AMK_ERR_INVALID_ARG : AMK_OK;
}
// The record of a checked frame that a slot keeps until its gang is launched
amk_pipeline::Staged staged(const amk_pipeline_frame &f) {
    amk_pipeline::Staged o;
    o.frame = f;
    if (f.n_keyframes > 0) {
        o.kf_obstacle.assign(f.kf_obstacle, f.kf_obstacle + f.n_keyframes);
        o.kf_edge.assign(f.kf_edge, f.kf_edge + f.n_keyframes);
    }
    o.has_camera = f.camera != nullptr;
    if (f.camera) o.camera = *f.camera;
    o.input_ready = (hipEvent_t)f.input_ready;
    o.frame.kf_obstacle = o.frame.kf_edge = nullptr; o.frame.camera = nullptr;   // (the caller's host storage: a launch reads the copies)
    return o;
}
}  // namespace

extern "C" {
int amk_pipeline_create(const amk_pipeline_config *cfg, amk_pipeline **out) {
    if (!cfg || !out || cfg->n_slots <= 0 || cfg->n_slots > AMK_PIPELINE_MAX_SLOTS || cfg->n_scenes <= 0 ||
        cfg->max_points <= 0 || cfg->max_edge_points <= 0 || cfg->gang < 0 || cfg->gang > AMK_PIPELINE_MAX_GANG ||
        cfg->step.mpc_max_iter < 1 || cfg->step.mpc_max_iter > AMK_MAX_OUTER_ITER || cfg->keyframes.max_frame_count < 0 ||
        (cfg->task.task != AMK_TASK_FORWARD && cfg->task.task != AMK_TASK_GLOBAL_GOAL))
        return AMK_ERR_INVALID_ARG;
    *out = nullptr;
    if (amk_device_count() <= 0) return AMK_ERR_NO_DEVICE;
    amk_pipeline *p = new amk_pipeline();
    p->cfg = *cfg;
    p->depth = cfg->queue_depth > 0 ? cfg->queue_depth : AMK_PIPELINE_DEFAULT_DEPTH;
    if (p->depth > AMK_PIPELINE_MAX_DEPTH) p->depth = AMK_PIPELINE_MAX_DEPTH;
    p->gang = cfg->gang > 0 ? cfg->gang : 1;
    p->slots.resize(cfg->n_slots);
    // one hardware queue per slot where the runtime's pool is too small for it (queue_policy, above)
    int least = 0, greatest = 0;   // numerically: greatest <= least (lower numbers are higher priorities)
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least < greatest) least = greatest = 0;
    int mode[AMK_PIPELINE_MAX_SLOTS], cls[AMK_PIPELINE_MAX_SLOTS];
    amk__pipeline_queue_policy(env_int("GPU_MAX_HW_QUEUES", 4), cfg->n_slots, least - greatest + 1, forced_queue_mode(), mode, cls);
    const bool fail_queue = g_fail_queue_creation != 0;
    g_fail_queue_creation = 0;
    for (int i = 0; i < cfg->n_slots; ++i)
        if (const int st = create_slot(p, p->slots[i], mode[i], greatest + cls[i], fail_queue); st != AMK_OK) {
            amk_pipeline_destroy(p);
            return st;
        }
    *out = p;
    return AMK_OK;
}

// The policy itself (pure; internal, exported for its test): how each of n_slots slots gets its stream when the runtime's pool
// holds `pool` hardware queues per priority class and the device has n_classes classes.  forced: AMK_QUEUES_* or -1 (automatic).
//   pooled     every slot takes a stream from the pool.  Automatic mode picks it when the pool has a queue for every slot and
//              one for the host's own stream (pool >= n_slots + 1) -- the configuration the documentation asks the host for --
//              and when the pool already holds AMK_PIPELINE_MAX_OWN_QUEUES queues (nothing may be added).
//   priority   the slots cycle over the classes (0 = the highest priority) in the order normal, low, high, so that every class's
//              own pool serves at most `pool` slots; slots beyond n_classes x pool, or beyond AMK_PIPELINE_MAX_OWN_QUEUES, are
//              pooled (they share).  The order matters, because the dispatcher honours the classes: a slot of a higher class
//              takes the CUs first, and the host's round robin then waits for the slots of the lower ones.  Of the six orders
//              this one leaves the high class the fewest slots and is the fastest on the bench's cold line by 6 - 13 %
//              (profiles/pipeline_queues_ab.txt section 3).
// mode_out / class_out: [n_slots].  Returns the number of slots that are not pooled.
int amk__pipeline_queue_policy(int pool, int n_slots, int n_classes, int forced, int *mode_out, int *class_out) {
    if (pool < 1 || n_slots < 1 || !mode_out || !class_out) return -1;
    if (n_classes < 1) n_classes = 1;
    int mode = forced;
    if (mode != AMK_QUEUES_POOLED && mode != AMK_QUEUES_PRIORITY)
        mode = (pool >= n_slots + 1 || pool >= AMK_PIPELINE_MAX_OWN_QUEUES) ? AMK_QUEUES_POOLED : AMK_QUEUES_PRIORITY;
    int own = 0;
    if (mode == AMK_QUEUES_PRIORITY) own = (int)std::min<long long>(std::min(n_slots, AMK_PIPELINE_MAX_OWN_QUEUES), (long long)n_classes * pool);
    const int normal = (n_classes - 1) / 2;   // the class of a stream created without a priority (the range is symmetric about it)
    for (int i = 0; i < n_slots; ++i) {
        mode_out[i] = i < own ? AMK_QUEUES_PRIORITY : AMK_QUEUES_POOLED;
        // the cycle: normal, the lower classes, then the higher ones from just above normal up to the highest
        const int k = i % n_classes;
        class_out[i] = i < own ? (k < n_classes - normal ? normal + k : n_classes - 1 - k) : normal;
    }
    return own;
}

int amk_pipeline_queue_mode(const amk_pipeline *p, int slot) {
    return (p && slot >= 0 && slot < (int)p->slots.size()) ? p->slots[slot].queue_mode : -1;
}

int amk_pipeline_destroy(amk_pipeline *p) {
    if (!p) return AMK_ERR_INVALID_ARG;
    for (auto &s : p->slots) {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        if (s.obstacle) amk_kd_destroy(s.obstacle);
        if (s.edge) amk_kd_destroy(s.edge);
        if (s.mpc) amk_mpc_destroy(s.mpc);
        if (s.map) amk_kfmap_destroy(s.map);
        for (auto ev : s.done)
            if (ev) (void)hipEventDestroy(ev);
        if (s.stream) (void)hipStreamDestroy(s.stream);
    }
    delete p;
    return AMK_OK;
}

int amk_pipeline_slots(const amk_pipeline *p) { return p ? (int)p->slots.size() : -1; }
int amk_pipeline_gang(const amk_pipeline *p) { return p ? p->gang : -1; }
amk_mpc *amk_pipeline_mpc(amk_pipeline *p, int slot) { const Slot *s = slot_at(p, slot); return s ? s->mpc : nullptr; }
amk_kfmap *amk_pipeline_kfmap(amk_pipeline *p, int slot) { const Slot *s = slot_at(p, slot); return s ? s->map : nullptr; }
void *amk_pipeline_stream(amk_pipeline *p, int slot) { const Slot *s = slot_at(p, slot); return s ? (void *)s->stream : nullptr; }
amk_kd *amk_pipeline_kd(amk_pipeline *p, int slot, int which) {
    const Slot *s = slot_at(p, slot);
    return !s ? nullptr : (which == 0 ? s->obstacle : (which == 1 ? s->edge : nullptr));
}

int amk_pipeline_submit(amk_pipeline *p, const amk_pipeline_frame *f, int *ticket_out) {
    if (!p || !f) return AMK_ERR_INVALID_ARG;
    if (const int st = frame_args(p->cfg, f); st != AMK_OK) return st;
    const int si = p->next, ns = (int)p->slots.size();
    Slot &s = p->slots[si];
    // the slot's own map: no caller keyframes; cloud frames bring mCurFrame.Twc AND the camera model -- the reference always runs
    // PtIsInFrame (FrameKDMap.cpp:339-345); without a camera every reference point would count as inside the current frame and
    // the keyframes would never be merged
    if (s.map && (f->n_keyframes > 0 || (!f->d_depth && (!f->d_Twc_cur || !f->camera)))) return AMK_ERR_INVALID_ARG;
    if (s.map && !s.open.empty()) {   // the map step takes ONE camera model per launch (position 0's): a gang must agree on it
        const amk_pipeline::Staged &o = s.open[0];
        if ((o.frame.d_depth != nullptr) != (f->d_depth != nullptr)) return AMK_ERR_INVALID_ARG;
        if (f->d_depth && (o.frame.depth_rows != f->depth_rows || o.frame.depth_cols != f->depth_cols)) return AMK_ERR_INVALID_ARG;
        if (!f->d_depth && std::memcmp(&o.camera, f->camera, sizeof(amk_frame_camera)) != 0) return AMK_ERR_INVALID_ARG;
    }
    if (f->n_keyframes > 0) {
        if (p->audit_mode != AMK_AUDIT_OFF) return AMK_ERR_UNSUPPORTED;   // the audit runs against the slot's own index or map only
        if (p->gang != 1) return AMK_ERR_UNSUPPORTED;   // keyframe handles hold n_scenes scenes, a gang's handles gang x n_scenes
        if (!f->kf_obstacle || !f->kf_edge) return AMK_ERR_INVALID_ARG;
        for (int i = 0; i < f->n_keyframes; ++i)
            if (!f->kf_obstacle[i] || !f->kf_edge[i]) return AMK_ERR_INVALID_ARG;
    }
    // a TASK frame shifts the mRefPath the slot keeps for its position: there must be one (InitCircleState's role, :14-23)
    if (f->d_odom && !f->d_ref_path_init && !s.ref_inited[s.open.size() < AMK_PIPELINE_MAX_GANG ? s.open.size() : 0]) return AMK_ERR_INVALID_ARG;
    const int stride = f->d_depth ? 3 : (f->point_stride ? f->point_stride : 3);
    if (stride != 3 && stride != 4) return AMK_ERR_INVALID_ARG;
    if (!s.open.empty() && stride != s.point_stride) return AMK_ERR_INVALID_ARG;   // one point layout per gang
    if ((int)s.open.size() >= p->gang) return AMK_ERR_INVALID_ARG;                  // (cannot happen: a full gang is launched at once)
    // Flow control.  A slot's launches are ordered by its stream, so queuing the next one behind a running one is safe (same
    // handles, same workspaces, in order); submit() only blocks when `depth` launches of this slot are still unfinished --
    // the event about to be re-recorded belongs to the launch issued `depth` launches ago.  depth 1 = at most one launch per
    // slot on the device (every launch then pays the host's reaction time between its predecessor's end and its own start).
    if (s.open.empty() && s.count - s.waited >= p->depth) {
        Stopwatch watch;
        const int ws = wait_event(s.done[s.count % p->depth]);
        if (Stopwatch::on())
            fprintf(stderr, "amk_pipeline submit: waited %.0f us for the launch issued %d launches ago on slot %d\n", watch.lap(), p->depth, si);
        if (ws != AMK_OK) return ws;
        s.waited = s.count - p->depth + 1;
    }
    const int g = (int)s.open.size();
    s.point_stride = stride;
    s.open.push_back(staged(*f));
    if (ticket_out) *ticket_out = g * ns + si;
    ++p->submitted;
    if ((int)s.open.size() == p->gang) return launch_slot(p, s);
    return AMK_OK;
}

int amk_pipeline_wait(amk_pipeline *p, int ticket) {
    Slot *s = slot_of(p, ticket);
    if (!s) return AMK_ERR_INVALID_ARG;
    if (const int st = launch_slot(p, *s); st != AMK_OK) return st;   // a partly filled gang: launch it now
    if (s->waited < s->count) {   // the newest event implies all earlier ones (in-order stream)
        if (const int ws = wait_event(s->done[(s->count - 1) % p->depth]); ws != AMK_OK) return ws;
        s->waited = s->count;
    }
    return s->fail_status;   // AMK_OK unless the slot's newest launch failed half-way (its frames were dropped)
}

int amk_pipeline_wait_stream(amk_pipeline *p, int ticket, void *stream) {
    Slot *s = slot_of(p, ticket);
    if (!s) return AMK_ERR_INVALID_ARG;
    if (const int st = launch_slot(p, *s); st != AMK_OK) return st;
    if (s->count > 0) AMK_HIP(hipStreamWaitEvent((hipStream_t)stream, s->done[(s->count - 1) % p->depth], 0));
    return s->fail_status;
}

int amk_pipeline_query(amk_pipeline *p, int ticket) {  // 1 = finished (or idle), 0 = still running or staged, -1 error
    Slot *s = slot_of(p, ticket);
    if (!s) return -1;
    if (!s->open.empty()) return 0;
    if (s->fail_status != AMK_OK) return -1;   // the slot's newest launch failed half-way: its frames were dropped (wait() tells why)
    if (s->waited >= s->count) return 1;
    const hipError_t e = hipEventQuery(s->done[(s->count - 1) % p->depth]);
    if (e == hipSuccess) { s->waited = s->count; return 1; }
    return e == hipErrorNotReady ? 0 : -1;
}

int amk_pipeline_drain(amk_pipeline *p) {
    if (!p) return AMK_ERR_INVALID_ARG;
    int first_error = AMK_OK;   // every slot is launched and waited for even when one fails: drain() leaves nothing in flight
    for (auto &s : p->slots)   // every open gang first: a launch must not wait for the slots before it to finish
        if (const int st = launch_slot(p, s); st != AMK_OK && first_error == AMK_OK) first_error = st;
    for (int i = 0; i < (int)p->slots.size(); ++i)
        if (const int st = amk_pipeline_wait(p, i); st != AMK_OK && first_error == AMK_OK) first_error = st;
    return first_error;
}

// tests only: the next launch of this pipeline fails at stage 1 (after the gather of the small inputs, before the index
// builds) or 2 (after the builds, before the control step) with AMK_ERR_HIP.  Stage 3, with p == NULL: in the next
// amk_pipeline_create every priority / dedicated stream creation call fails (the slots fall back to pooled streams).
int amk__pipeline_inject_failure(amk_pipeline *p, int stage) {
    if (!p && stage == 3) { g_fail_queue_creation = 1; return AMK_OK; }   // (no pipeline yet: the next amk_pipeline_create's)
    if (!p || stage < 0 || stage > 2) return AMK_ERR_INVALID_ARG;
    p->inject_failure = stage;
    return AMK_OK;
}

// The audit's switch.  Valid only while nothing is staged or in flight: a launch reads the mode, the radius and the buffers.
int amk_pipeline_set_path_audit(amk_pipeline *p, int mode, double radius, int n_legs) {
    if (!p || p->slots.empty() || (mode != AMK_AUDIT_OFF && mode != AMK_AUDIT_REPORT && mode != AMK_AUDIT_SLOW_DOWN) || !(radius >= 0.0))
        return AMK_ERR_INVALID_ARG;
    const int N = amk_mpc_horizon(p->slots[0].mpc);
    if (n_legs < 0 || n_legs > N - 1 || N < 2) return AMK_ERR_INVALID_ARG;
    for (auto &s : p->slots) {
        if (!s.open.empty()) return AMK_ERR_UNSUPPORTED;
        if (s.waited < s.count) {   // finished without the host having asked yet?
            const hipError_t e = hipEventQuery(s.done[(s.count - 1) % p->depth]);
            if (e == hipErrorNotReady) {
                (void)hipGetLastError();   // (not a failure: nothing for the next launch's check to find)
                return AMK_ERR_UNSUPPORTED;
            }
            if (e != hipSuccess) return amk::hip_fail(e);
            s.waited = s.count;
        }
    }
    if (mode != AMK_AUDIT_OFF) {
        const size_t GS = (size_t)p->gang * p->cfg.n_scenes;
        for (auto &s : p->slots) {
            if (s.audit_stop.p) continue;   // (all six or none: a failed attempt released them)
            const hipError_t e = alloc_all(s.audit_stop, GS, s.audit_leg, GS, s.audit_src, GS, s.audit_t, GS, s.audit_free, GS, s.audit_pts, GS * 3);
            if (e != hipSuccess) {
                s.audit_stop.release(); s.audit_leg.release(); s.audit_src.release(); s.audit_t.release(); s.audit_free.release(); s.audit_pts.release();
                return amk::hip_fail(e);
            }
        }
    }
    p->audit_mode = mode;
    p->audit_radius_sq = radius * radius;
    p->audit_points = (n_legs > 0 ? n_legs : N - 1) + 1;
    return AMK_OK;
}

int amk_pipeline_audit_outputs(amk_pipeline *p, int ticket, int **d_stop, int **d_leg, double **d_t, double **d_free, float **d_pts,
                               int **d_src) {
    Slot *s = slot_of(p, ticket);
    if (!s) return AMK_ERR_INVALID_ARG;
    if (!s->audit_stop.p) return AMK_ERR_UNSUPPORTED;   // (no amk_pipeline_set_path_audit yet)
    const size_t o = (size_t)(ticket / (int)p->slots.size()) * p->cfg.n_scenes;
    if (d_stop) *d_stop = s->audit_stop.p + o;
    if (d_leg) *d_leg = s->audit_leg.p + o;
    if (d_t) *d_t = s->audit_t.p + o;
    if (d_free) *d_free = s->audit_free.p + o;
    if (d_pts) *d_pts = s->audit_pts.p + o * 3;
    if (d_src) *d_src = s->audit_src.p + o;
    return AMK_OK;
}

int amk_pipeline_outputs(amk_pipeline *p, int ticket, double **d_u, double **d_x0array, int **d_flags, double **d_ref_path) {
    Slot *s = slot_of(p, ticket);
    if (!s) return AMK_ERR_INVALID_ARG;
    const size_t S = p->cfg.n_scenes, N = amk_mpc_horizon(s->mpc), o = (size_t)(ticket / (int)p->slots.size()) * S;
    if (d_u) *d_u = s->u.p + o * 4;
    if (d_x0array) *d_x0array = s->x0array.p + o * N * 14;
    if (d_flags) *d_flags = s->flags.p + o * 4;
    if (d_ref_path) *d_ref_path = s->ref_path.p + o * N * 10;
    return AMK_OK;
}
}  // extern "C"
