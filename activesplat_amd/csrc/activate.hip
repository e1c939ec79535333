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

// Final pass of the camera-pose gradient: the per-workgroup rows summed in fp64 in a fixed order (thread t adds column t % 16 of rows
// t / 16, t / 16 + 16, ...; then the 16 slices in order), dL/dR turned into dL/dq_cam through build_rotation's normalisation and quat_to_rot's
// formula and added to the rotation term; out = dL/d(qw,qx,qy,qz,tx,ty,tz) of the pose7 the launch received.  One workgroup: the same numbers on every run.
__global__ __launch_bounds__(kBlock) void pose_grad_finish_kernel(int64_t nrows, Pose pose, const float* __restrict__ rows, float* __restrict__ out)
{
    constexpr int kSlices = kBlock / kPoseAcc;
    __shared__ double s[kSlices][kPoseAcc];
    const int c = threadIdx.x % kPoseAcc, sl = threadIdx.x / kPoseAcc;
    double acc = 0.0;
    for (int64_t r = sl; r < nrows; r += kSlices) acc += (double)rows[r * kPoseAcc + c];
    s[sl][c] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t[kPoseAcc];
    for (int k = 0; k < kPoseAcc; k++) {
        double v = 0.0;
        for (int j = 0; j < kSlices; j++) v += s[j][k];
        t[k] = v;
    }
    const double* dR = t + 3;            // row-major dL/dR
    // the reference builds the matrix as build_rotation(q) = R(q / |q|) (slam_external.py:25-42): dL/dR reaches q through quat_to_rot at the unit
    // quaternion AND that normalisation -- (I - u u^T) / |q| -- so the result is the reference's dL/dq for any q the caller chains it into
    // (a unit leaf passed as is included), not only after a further F.normalize.  (The rotation term is taken as quat_mult(q, .) takes it: as is.)
    const double q0 = pose.q[0], q1 = pose.q[1], q2 = pose.q[2], q3 = pose.q[3];
    const double nq = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const double r = q0 / nq, x = q1 / nq, y = q2 / nq, z = q3 / nq;
    const double d0 = 2.0 * (-z * dR[1] + y * dR[2] + z * dR[3] - x * dR[5] - y * dR[6] + x * dR[7]);
    const double d1 = 2.0 * (y * dR[1] + z * dR[2] + y * dR[3] - 2.0 * x * dR[4] - r * dR[5] + z * dR[6] + r * dR[7] - 2.0 * x * dR[8]);
    const double d2 = 2.0 * (-2.0 * y * dR[0] + x * dR[1] + r * dR[2] + x * dR[3] + z * dR[5] - r * dR[6] + z * dR[7] - 2.0 * y * dR[8]);
    const double d3 = 2.0 * (-2.0 * z * dR[0] - r * dR[1] + x * dR[2] + r * dR[3] - 2.0 * z * dR[4] + y * dR[5] + x * dR[6] + y * dR[7]);
    const double dot = r * d0 + x * d1 + y * d2 + z * d3;
    out[0] = (float)((d0 - r * dot) / nq + t[12]); out[1] = (float)((d1 - x * dot) / nq + t[13]);
    out[2] = (float)((d2 - y * dot) / nq + t[14]); out[3] = (float)((d3 - z * dot) / nq + t[15]);
    out[4] = (float)t[0]; out[5] = (float)t[1]; out[6] = (float)t[2];
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

hipError_t launch_pose_grad_finish(int64_t nrows, const float* pose7, const float* pose_rows, float* dpose7, hipStream_t st)
{
    Pose p; for (int k = 0; k < 4; k++) p.q[k] = pose7[k]; for (int k = 0; k < 3; k++) p.t[k] = pose7[4 + k];
    hipLaunchKernelGGL(pose_grad_finish_kernel, dim3(1), dim3(kBlock), 0, st, nrows, p, pose_rows, dpose7);
    return hipGetLastError();
}

}  // namespace gs
