// activate.hip -- fused frame transform + activations (forward and backward), one launch each.
//
// Replaces the ~15 elementwise / matmul torch kernels (and as many autograd nodes) the reference issues per
// render to build the rasteriser inputs:
//   transform_to_frame            src/mapper/splatam/utils/slam_helpers.py:252-304
//       means_cam = R(q_cam) p + t_cam ;  rot = quat_mult(q_cam, normalize(q))   (anisotropic; isotropic keeps q)
//   transformed_params2rendervar  slam_helpers.py:124-139
//       rotations = normalize(rot) ; opacities = sigmoid(logit) ; scales = exp(log_scales) (tiled x3 if isotropic)
// q_cam is the already-normalised camera quaternion (w,x,y,z).  HBM-bound streaming: 14 floats in, 11 out per Gaussian.
// Camera gradients (camera_grad=True, slam_helpers.py:270-271: tracking and bundle adjustment) come from the POSE instantiations of the backward:
// every Gaussian's share (pose_grad_accumulate, gs_common.h -- the per-Gaussian rasteriser backward uses the same helper) is summed per
// workgroup and the rows reduced in a fixed order by pose_grad_finish_kernel into dL/d(qw,qx,qy,qz,tx,ty,tz): bit-identical from run to run.
#include "gs_common.h"

namespace gs {

struct Pose { float q[4]; float t[3]; };

__global__ __launch_bounds__(kBlock) void activate_forward_kernel(int P, int iso, Pose pose, const float* __restrict__ means3D,
                                                                  const float* __restrict__ rots, const float* __restrict__ logit_op,
                                                                  const float* __restrict__ log_scales, float* __restrict__ o_means,
                                                                  float* __restrict__ o_rots, float* __restrict__ o_op,
                                                                  float* __restrict__ o_scales)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    float R[3][3];
    quat_to_rot(pose.q, R);
    const float px = means3D[3 * i], py = means3D[3 * i + 1], pz = means3D[3 * i + 2];
    o_means[3 * i] = R[0][0] * px + R[0][1] * py + R[0][2] * pz + pose.t[0];
    o_means[3 * i + 1] = R[1][0] * px + R[1][1] * py + R[1][2] * pz + pose.t[1];
    o_means[3 * i + 2] = R[2][0] * px + R[2][1] * py + R[2][2] * pz + pose.t[2];
    const float4 q4 = reinterpret_cast<const float4*>(rots)[i];
    const float q[4] = {q4.x, q4.y, q4.z, q4.w};
    float out[4];
    if (iso) {
        const float inv = 1.0f / fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
        for (int k = 0; k < 4; k++) out[k] = q[k] * inv;
    } else {
        const float inv = 1.0f / fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
        const float u[4] = {q[0] * inv, q[1] * inv, q[2] * inv, q[3] * inv};
        float m[4];
        qmul(pose.q, u, m);
        const float invm = 1.0f / fmaxf(sqrtf(m[0] * m[0] + m[1] * m[1] + m[2] * m[2] + m[3] * m[3]), 1e-12f);
        for (int k = 0; k < 4; k++) out[k] = m[k] * invm;
    }
    reinterpret_cast<float4*>(o_rots)[i] = make_float4(out[0], out[1], out[2], out[3]);
    o_op[i] = 1.0f / (1.0f + __expf(-logit_op[i]));
    if (iso) {
        const float s = __expf(log_scales[i]);
        o_scales[3 * i] = s; o_scales[3 * i + 1] = s; o_scales[3 * i + 2] = s;
    } else {
        o_scales[3 * i] = __expf(log_scales[3 * i]); o_scales[3 * i + 1] = __expf(log_scales[3 * i + 1]);
        o_scales[3 * i + 2] = __expf(log_scales[3 * i + 2]);
    }
}

// ACC: the four outputs are ADDED to what d_* already hold (gradient accumulation over the keyframes of a batch in the kernel that produces
// the gradient: the separate `grad += new` passes of autograd move 3 x 44 bytes per Gaussian and keyframe)
// POSE (camera-pose gradient; means3D = the world-frame means): 1 = every Gaussian also adds its share (pose_grad_accumulate, gs_common.h -- the
// per-Gaussian rasteriser backward uses the same helper) to a per-thread record, and every workgroup writes one row of kPoseAcc partial sums to
// pose_rows (no float atomics; pose_grad_finish_kernel reduces the rows in a fixed order); 2 = ONLY that share: no d_* row is written, none of
// the parameter-side chain runs.  A row whose incoming means / rotation gradients are all zero adds nothing to the pose: that is what the
// rasteriser hands a Gaussian it did not render, whose parameters may be non-finite (0 x NaN would poison the whole sum).
template <bool ACC, int POSE = 0>
__global__ __launch_bounds__(kBlock) void activate_backward_kernel(int P, int iso, Pose pose, const float* __restrict__ rots,
                                                                   const float* __restrict__ o_op, const float* __restrict__ o_scales,
                                                                   const float* __restrict__ g_means, const float* __restrict__ g_rots,
                                                                   const float* __restrict__ g_op, const float* __restrict__ g_scales,
                                                                   float* __restrict__ d_means, float* __restrict__ d_rots,
                                                                   float* __restrict__ d_logit, float* __restrict__ d_logs,
                                                                   const float* __restrict__ means3D, float* __restrict__ pose_rows)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    float pacc[kPoseAcc];
    for (int k = 0; k < kPoseAcc; k++) pacc[k] = 0.f;
    {
    if (i >= P) { if (POSE != 0) goto pose_reduce; return; }
    float R[3][3];
    quat_to_rot(pose.q, R);
    const float gx = g_means ? g_means[3 * i] : 0.f, gy = g_means ? g_means[3 * i + 1] : 0.f, gz = g_means ? g_means[3 * i + 2] : 0.f;
    if (POSE != 0) {
        const float4 t4 = reinterpret_cast<const float4*>(rots)[i];
        const float qp[4] = {t4.x, t4.y, t4.z, t4.w};
        float gp[4] = {0.f, 0.f, 0.f, 0.f};
        if (g_rots) { const float4 t = reinterpret_cast<const float4*>(g_rots)[i]; gp[0] = t.x; gp[1] = t.y; gp[2] = t.z; gp[3] = t.w; }
        if (gx != 0.f || gy != 0.f || gz != 0.f || gp[0] != 0.f || gp[1] != 0.f || gp[2] != 0.f || gp[3] != 0.f) {
            const float w[3] = {means3D[3 * i], means3D[3 * i + 1], means3D[3 * i + 2]};
            const float dmean[3] = {gx, gy, gz};
            pose_grad_accumulate(pose.q, iso, w, dmean, qp, gp, pacc);
        }
        if (POSE == 2) goto pose_reduce;
    }
    const float m0 = R[0][0] * gx + R[1][0] * gy + R[2][0] * gz, m1 = R[0][1] * gx + R[1][1] * gy + R[2][1] * gz,
                m2 = R[0][2] * gx + R[1][2] * gy + R[2][2] * gz;
    d_means[3 * i] = ACC ? d_means[3 * i] + m0 : m0;
    d_means[3 * i + 1] = ACC ? d_means[3 * i + 1] + m1 : m1;
    d_means[3 * i + 2] = ACC ? d_means[3 * i + 2] + m2 : m2;
    // rotations
    const float4 q4 = reinterpret_cast<const float4*>(rots)[i];
    const float q[4] = {q4.x, q4.y, q4.z, q4.w};
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (g_rots) { const float4 t = reinterpret_cast<const float4*>(g_rots)[i]; g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w; }
    const float nq = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
    const float u[4] = {q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq};
    float du[4];
    if (iso) {
        for (int k = 0; k < 4; k++) du[k] = g[k];
    } else {
        float m[4];
        qmul(pose.q, u, m);
        const float nm = fmaxf(sqrtf(m[0] * m[0] + m[1] * m[1] + m[2] * m[2] + m[3] * m[3]), 1e-12f);
        const float r[4] = {m[0] / nm, m[1] / nm, m[2] / nm, m[3] / nm};
        const float dot = r[0] * g[0] + r[1] * g[1] + r[2] * g[2] + r[3] * g[3];
        float dm[4];
        for (int k = 0; k < 4; k++) dm[k] = (g[k] - r[k] * dot) / nm;
        qmul_bwd_rhs(pose.q, dm, du);
    }
    const float dotu = u[0] * du[0] + u[1] * du[1] + u[2] * du[2] + u[3] * du[3];
    float4 dq = make_float4((du[0] - u[0] * dotu) / nq, (du[1] - u[1] * dotu) / nq, (du[2] - u[2] * dotu) / nq, (du[3] - u[3] * dotu) / nq);
    if (ACC) { const float4 old = reinterpret_cast<const float4*>(d_rots)[i]; dq.x += old.x; dq.y += old.y; dq.z += old.z; dq.w += old.w; }
    reinterpret_cast<float4*>(d_rots)[i] = dq;
    const float o = o_op[i];
    const float dlg = (g_op ? g_op[i] : 0.f) * o * (1.0f - o);
    d_logit[i] = ACC ? d_logit[i] + dlg : dlg;
    const float s0 = g_scales ? g_scales[3 * i] * o_scales[3 * i] : 0.f, s1 = g_scales ? g_scales[3 * i + 1] * o_scales[3 * i + 1] : 0.f,
                s2 = g_scales ? g_scales[3 * i + 2] * o_scales[3 * i + 2] : 0.f;
    if (iso) d_logs[i] = ACC ? d_logs[i] + (s0 + s1 + s2) : s0 + s1 + s2;
    else {
        d_logs[3 * i] = ACC ? d_logs[3 * i] + s0 : s0; d_logs[3 * i + 1] = ACC ? d_logs[3 * i + 1] + s1 : s1;
        d_logs[3 * i + 2] = ACC ? d_logs[3 * i + 2] + s2 : s2;
    }
    }
    if (POSE == 0) return;
pose_reduce:
    if (POSE != 0) pose_grad_block_row(pacc, pose_rows + (size_t)blockIdx.x * kPoseAcc);
}

// Final pass of the camera-pose gradient (pose_grad_finish_block, gs_common.h): out = dL/d(qw,qx,qy,qz,tx,ty,tz) of the pose7 the launch received.
// One workgroup: the same numbers on every run.
__global__ __launch_bounds__(kBlock) void pose_grad_finish_kernel(int64_t nrows, Pose pose, const float* __restrict__ rows, float* __restrict__ out)
{
    pose_grad_finish_block(nrows, pose, rows, out);
}

// The same with the pose read from the device column (the device-pose backward, gs_render_backward_raw_pose_dev): dL/d of the normalised column.
__global__ __launch_bounds__(kBlock) void pose_grad_finish_dev_kernel(int64_t nrows, const float* __restrict__ dev_q, int64_t stride,
                                                                      const float* __restrict__ rows, float* __restrict__ out)
{
    Pose p;
    float n;
    normalize_pose_column(dev_q, stride, p.q, n);
    pose_grad_finish_block(nrows, p, rows, out);
}

// ---- tracking (SplaTAM's per-frame pose optimisation, torch.optim.Adam on cam_unnorm_rots[..., t] / cam_trans[..., t]) ----
// state (kTrackState floats, gs_tracking_state_bytes): [0,7) first moments, [7,14) second moments, [14] the smallest loss so far, [15,22) the
// candidate pose (the column after the step of that iteration), [22,25) the last iteration's {loss, depth, im}, [25] steps skipped
__global__ void tracking_begin_kernel(const float* __restrict__ rots_col, const float* __restrict__ trans_col, int64_t stride,
                                      float* __restrict__ state)
{
    const int k = threadIdx.x;
    if (k >= kTrackState) return;
    float v = 0.f;
    if (k == 14) v = 1e20f;                                        // SplaTAM's current_min_loss = float(1e20)
    else if (k >= 15 && k < 19) v = rots_col[(k - 15) * stride];  // the candidate starts as the initial pose
    else if (k >= 19 && k < 22) v = trans_col[(k - 19) * stride];
    state[k] = v;
}

// One tracking iteration's tail, one workgroup, after the pose-only backward: (1) the loss rows reduced in fp64 in a fixed order, (2) the pose
// rows reduced exactly as pose_grad_finish_kernel reduces them, at the normalised column, then taken through F.normalize's Jacobian at the
// unnormalised column (dL/dcam_unnorm_rots[..., t] as autograd delivers it), (3) torch.optim.Adam's step on the 7 values in place (torch's fp32
// operation order of the foreach path; skipped, with the candidate, while a chained backward in front has failed -- Cam::chain_fail), (4) the
// best candidate: loss < min_loss (strict: the first minimum wins, a NaN never does) -> min_loss = loss, candidate = the column AFTER this step,
// (5) the last losses and, if asked, a history row {loss, depth, im, 7 post-step values}.
__global__ __launch_bounds__(kBlock) void tracking_step_kernel(int64_t pose_nrows, const float* __restrict__ pose_rows, int64_t loss_nrows,
                                                               const float* __restrict__ loss_rows, float w_im, float w_depth,
                                                               float* __restrict__ rots_col, float* __restrict__ trans_col, int64_t stride,
                                                               TrackAdam c, float* __restrict__ state, float* __restrict__ history_row,
                                                               const uint32_t* __restrict__ fail)
{
    float L[3];
    tracking_loss_reduce(loss_nrows, loss_rows, w_im, w_depth, L);       // (all threads; thread 0 comes back with L)
    __syncthreads();
    Pose pu;                                                             // the normalised column (the pose the rows were formed at)
    float norm;
    normalize_pose_column(rots_col, stride, pu.q, norm);
    const float* u = pu.q;
    double g[7];                                                         // (unrounded: the whole chain is double, the gradient is rounded once)
    pose_grad_finish_block(pose_nrows, pu, pose_rows, g);                 // (all threads; thread 0 comes back with g)
    if (threadIdx.x != 0) return;
    // F.normalize backward: x / max(|x|, eps) -> dL/dx = (g - u (u . g)) / |x|  (|x| below eps: the clamp passes g / eps)
    const double n = norm, ug = (double)u[0] * g[0] + (double)u[1] * g[1] + (double)u[2] * g[2] + (double)u[3] * g[3];
    float grad[7];
    for (int k = 0; k < 4; k++) grad[k] = n >= 1e-12 ? (float)((g[k] - (double)u[k] * ug) / n) : (float)(g[k] / 1e-12);
    for (int k = 4; k < 7; k++) grad[k] = (float)g[k];
    float p[7];
    for (int k = 0; k < 4; k++) p[k] = rots_col[k * stride];
    for (int k = 0; k < 3; k++) p[4 + k] = trans_col[k * stride];
    const bool skip = chain_failed(fail);
    if (!skip) {
#pragma clang fp contract(off)
        for (int k = 0; k < 7; k++) {
            float m = state[k], v = state[7 + k];
            m = m + c.one_m_b1 * (grad[k] - m);                          // exp_avg.lerp_(grad, 1 - beta1)
            v = v * c.b2;                                                 // exp_avg_sq.mul_(beta2)
            v = v + c.one_m_b2 * (grad[k] * grad[k]);                     //           .addcmul_(grad, grad, 1 - beta2)
            const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;            // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
            p[k] = p[k] + c.neg_step_size[k < 4 ? 0 : 1] * (m / denom);  // param.addcdiv_(exp_avg, denom, -lr / bias_correction1)
            state[k] = m; state[7 + k] = v;
        }
        for (int k = 0; k < 4; k++) rots_col[k * stride] = p[k];
        for (int k = 0; k < 3; k++) trans_col[k * stride] = p[4 + k];
        if (L[0] < state[14]) {
            state[14] = L[0];
            for (int k = 0; k < 7; k++) state[15 + k] = p[k];
        }
    } else {
        state[25] = state[25] + 1.f;
    }
    state[22] = L[0]; state[23] = L[1]; state[24] = L[2];
    if (history_row) {
        for (int k = 0; k < 3; k++) history_row[k] = L[k];
        for (int k = 0; k < 7; k++) history_row[3 + k] = p[k];
    }
}

hipError_t launch_activate_forward(int P, int iso, const float* pose7, const float* means3D, const float* rots, const float* logit_op,
                                   const float* log_scales, float* o_means, float* o_rots, float* o_op, float* o_scales, hipStream_t st)
{
    Pose p; for (int k = 0; k < 4; k++) p.q[k] = pose7[k]; for (int k = 0; k < 3; k++) p.t[k] = pose7[4 + k];
    const int nb = (P + kBlock - 1) / kBlock;
    if (nb > 0) hipLaunchKernelGGL(activate_forward_kernel, dim3(nb), dim3(kBlock), 0, st, P, iso, p, means3D, rots, logit_op, log_scales,
                                   o_means, o_rots, o_op, o_scales);
    return hipGetLastError();
}

hipError_t launch_activate_backward(int P, int iso, const float* pose7, const float* rots, const float* o_op, const float* o_scales,
                                    const float* g_means, const float* g_rots, const float* g_op, const float* g_scales, float* d_means,
                                    float* d_rots, float* d_logit, float* d_logs, int accumulate, hipStream_t st)
{
    Pose p; for (int k = 0; k < 4; k++) p.q[k] = pose7[k]; for (int k = 0; k < 3; k++) p.t[k] = pose7[4 + k];
    const int nb = (P + kBlock - 1) / kBlock;
    if (nb > 0 && accumulate)
        hipLaunchKernelGGL(activate_backward_kernel<true>, dim3(nb), dim3(kBlock), 0, st, P, iso, p, rots, o_op, o_scales, g_means, g_rots,
                           g_op, g_scales, d_means, d_rots, d_logit, d_logs, nullptr, nullptr);
    else if (nb > 0)
        hipLaunchKernelGGL(activate_backward_kernel<false>, dim3(nb), dim3(kBlock), 0, st, P, iso, p, rots, o_op, o_scales, g_means, g_rots,
                           g_op, g_scales, d_means, d_rots, d_logit, d_logs, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_activate_backward_pose(int P, int iso, const float* pose7, const float* means3D, const float* rots, const float* o_op,
                                         const float* o_scales, const float* g_means, const float* g_rots, const float* g_op,
                                         const float* g_scales, float* d_means, float* d_rots, float* d_logit, float* d_logs, int accumulate,
                                         int pose_mode, float* pose_rows, hipStream_t st)
{
    if (pose_mode < 1 || pose_mode > 2) return hipErrorInvalidValue;
    Pose p; for (int k = 0; k < 4; k++) p.q[k] = pose7[k]; for (int k = 0; k < 3; k++) p.t[k] = pose7[4 + k];
    const int nb = (P + kBlock - 1) / kBlock;
#define GS_ABWD_POSE(A_, M_) hipLaunchKernelGGL((activate_backward_kernel<A_, M_>), dim3(nb), dim3(kBlock), 0, st, P, iso, p, rots, o_op, o_scales, \
                                                g_means, g_rots, g_op, g_scales, d_means, d_rots, d_logit, d_logs, means3D, pose_rows)
    if (nb > 0 && pose_mode == 2) GS_ABWD_POSE(false, 2);
    else if (nb > 0 && accumulate) GS_ABWD_POSE(true, 1);
    else if (nb > 0) GS_ABWD_POSE(false, 1);
#undef GS_ABWD_POSE
    return hipGetLastError();
}

hipError_t launch_pose_grad_finish_dev(int64_t nrows, const float* dev_q, int64_t stride, const float* pose_rows, float* dpose7, hipStream_t st)
{
    hipLaunchKernelGGL(pose_grad_finish_dev_kernel, dim3(1), dim3(kBlock), 0, st, nrows, dev_q, stride, pose_rows, dpose7);
    return hipGetLastError();
}

hipError_t launch_tracking_begin(const float* rots_col, const float* trans_col, int64_t stride, float* state, hipStream_t st)
{
    hipLaunchKernelGGL(tracking_begin_kernel, dim3(1), dim3(kTrackState), 0, st, rots_col, trans_col, stride, state);
    return hipGetLastError();
}

hipError_t launch_tracking_step(int64_t pose_nrows, const float* pose_rows, int64_t loss_nrows, const float* loss_rows, float w_im, float w_depth,
                                float* rots_col, float* trans_col, int64_t stride, const TrackAdam& c, float* state, float* history_row,
                                hipStream_t st)
{
    hipLaunchKernelGGL(tracking_step_kernel, dim3(1), dim3(kBlock), 0, st, pose_nrows, pose_rows, loss_nrows, loss_rows, w_im, w_depth,
                       rots_col, trans_col, stride, c, state, history_row, (const uint32_t*)chain_fail_word());
    return hipGetLastError();
}

hipError_t launch_pose_grad_finish(int64_t nrows, const float* pose7, const float* pose_rows, float* dpose7, hipStream_t st)
{
    Pose p; for (int k = 0; k < 4; k++) p.q[k] = pose7[k]; for (int k = 0; k < 3; k++) p.t[k] = pose7[4 + k];
    hipLaunchKernelGGL(pose_grad_finish_kernel, dim3(1), dim3(kBlock), 0, st, nrows, p, pose_rows, dpose7);
    return hipGetLastError();
}

}  // namespace gs
