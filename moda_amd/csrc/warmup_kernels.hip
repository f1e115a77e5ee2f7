// What the reference runs before the first forward_default call (scripts/template.sh: --warmup_shape_ep 5 --warmup_rootmlp), the
// thin part around the networks, device-resident: no host synchronisation, no allocation, every launch on the caller's stream, so a
// warm-up step can be captured into one graph.
//
//   shape target   (nnutils/loss_utils.py:546-563 shape_init_loss)  one thread per point: the sample (u * 2) * bound - bound in three
//                  separately rounded fp32 operations, and its signed distance to the ellipsoid / sphere of the object bound.
//   shape loss     (:570-571)  mean((-y - dis)^2): block partials in float64, one workgroup sums them in index order; the backward
//                  is one thread per element and reads the incoming gradient from device memory; on request it also leaves
//                  sum(dy) -- the gradient of a bias directly in front of y -- formed by the same fixed tree.
//   rtk loss       (:151-163 rtk_loss, geom_utils.py:1196-1205 rot_angle)  one workgroup forward; every frame's gradient depends on
//                  that frame alone, so the backward is one thread per frame.
//   root smoothness, first order  (:520-537 compute_root_sm_loss)  one workgroup forward; the backward is a gather: one thread per
//                  frame sums the up to two pairs the frame belongs to, in a fixed order.
//   matrix -> quaternion  (train_utils.py:664-666, pytorch3d's matrix_to_quaternion restated)  one thread per matrix.
// No float atomics anywhere: for given inputs every sum has one fixed tree (lanes by wave_add's xor butterfly 32..1, waves in index
// order through LDS; the one-workgroup pose forwards through block_sums of pose_loss.h, which this file shares with
// lossasm_kernels.hip).  Device memory is written by plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "moda_dev.h"
#include "pose_loss.h"

#pragma clang fp contract(off)

namespace {

// ---- shape initialisation ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void shape_target_kernel(const float* __restrict__ u, long long N, const float* __restrict__ obj_bound,
                                                           float bound_factor, int ellips, float* __restrict__ pts,
                                                           float* __restrict__ dis) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float ob[3] = {obj_bound[0], obj_bound[1], obj_bound[2]};
    float p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float b = ob[k] * bound_factor;
        const float t = u[3 * i + k] * 2.f;                        // three roundings, as torch.rand(...) * 2 * bound - bound
        const float m = t * b;
        p[k] = m - b;
        pts[3 * i + k] = p[k];
    }
    float d;
    if (ellips) {
        const float q0 = __fdiv_rn(p[0], ob[0]), q1 = __fdiv_rn(p[1], ob[1]), q2 = __fdiv_rn(p[2], ob[2]);
        const float s = (q0 * q0 + q1 * q1) + q2 * q2;
        const float mean = __fdiv_rn((ob[0] + ob[1]) + ob[2], 3.f);
        d = (sqrtf(s) - 1.f) * mean;
    } else {
        const float s = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
        d = sqrtf(s) - fminf(fminf(ob[0], ob[1]), ob[2]);
    }
    dis[i] = d;
}

// SQ: the terms are the squares r r of r = -a - b (the loss); else the values of a (a gradient's ordered sum)
template <bool SQ>
__global__ __launch_bounds__(256) void sum_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, long long N,
                                                          double* __restrict__ partials) {
    __shared__ double sh[4];
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
        if (SQ) {
            const float r = -a[i] - b[i];
            s += (double)(r * r);
        } else {
            s += (double)a[i];
        }
    }
    s = wave_add(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// out[0] = (float)(sum of the partials / div)
__global__ __launch_bounds__(1024) void sum_final_kernel(const double* __restrict__ partials, int nb, double div, float* __restrict__ out) {
    __shared__ double sh[16];
    double s = (int)threadIdx.x < nb ? partials[threadIdx.x] : 0.0;
    s = wave_add(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += sh[w];
        out[0] = (float)(t / div);
    }
}

__global__ __launch_bounds__(256) void shape_loss_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dis, long long N,
                                                             const float* __restrict__ g, float* __restrict__ dy) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float c = __fdiv_rn(g[0], (float)N);
    const float r = -y[i] - dis[i];
    dy[i] = -(c * (2.f * r));
}

// ---- poses ---------------------------------------------------------------------------------------------------------------
// out[0] = rot_loss + trn_loss, out[1] = rot_loss = 0.01 * mean(angle), out[2] = trn_loss = mean |tp - tg|^2
__global__ __launch_bounds__(1024) void rtk_loss_fwd_kernel(const float* __restrict__ rtk, int stride, const float* __restrict__ gt,
                                                            int stride_gt, int T, float* __restrict__ out) {
    __shared__ double sh_a[16], sh_t[16];
    __shared__ int sh_c[16];
    double sa = 0.0, st = 0.0;
    int cnt = 0;
    for (int f = threadIdx.x; f < T; f += blockDim.x) {
        float Rp[9], Rg[9], tp[3], tg[3];
        load_pose(rtk, stride, f, Rp, tp);
        load_pose(gt, stride_gt, f, Rg, tg);
        sa += (double)angle_of(cos_of(Rp, Rg));
        const float d0 = tp[0] - tg[0], d1 = tp[1] - tg[1], d2 = tp[2] - tg[2];
        st += (double)((d0 * d0 + d1 * d1) + d2 * d2);
        cnt += 1;
    }
    block_sums<16>(sa, st, cnt, sh_a, sh_t, sh_c);
    if (threadIdx.x == 0) {
        const float rot = 0.01f * (float)(sa / (double)cnt);
        const float trn = (float)(st / (double)cnt);
        out[0] = rot + trn;
        out[1] = rot;
        out[2] = trn;
    }
}

// g_total, g_rot, g_trn: the gradients of the three outputs (a NULL one is zero)
__global__ __launch_bounds__(256) void rtk_loss_bwd_kernel(const float* __restrict__ rtk, int stride, const float* __restrict__ gt,
                                                           int stride_gt, int T, const float* __restrict__ g_total,
                                                           const float* __restrict__ g_rot, const float* __restrict__ g_trn,
                                                           float* __restrict__ drtk) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= T) return;
    const float gt0 = g_total ? g_total[0] : 0.f;
    const float gr = gt0 + (g_rot ? g_rot[0] : 0.f), gn = gt0 + (g_trn ? g_trn[0] : 0.f);
    float Rp[9], Rg[9], tp[3], tg[3], dR[9], dt[3];
    load_pose(rtk, stride, f, Rp, tp);
    load_pose(gt, stride_gt, f, Rg, tg);
    // cos = <Rp, Rg> / 2 - 1/2: d cos / d Rp = Rg / 2
    const float gc = gr * 0.01f / (float)T * dangle_of(cos_of(Rp, Rg)) * 0.5f;
    const float ct = gn / (float)T * 2.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) dR[i] = gc * Rg[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) dt[c] = ct * (tp[c] - tg[c]);
    store_pose_grad(drtk, stride, f, dR, dt);
}

struct Pair {
    float R0[9], R1[9], d[3];
    float cosv, trn;
};

DEVINL void pair_eval(const float* __restrict__ rtk, int stride, long long j, Pair& q) {
    float t0[3], t1[3];
    load_pose(rtk, stride, j, q.R0, t0);
    load_pose(rtk, stride, j + 1, q.R1, t1);
    q.cosv = cos_of(q.R0, q.R1);
#pragma unroll
    for (int c = 0; c < 3; ++c) q.d[c] = t0[c] - t1[c];
    q.trn = sqrtf((q.d[0] * q.d[0] + q.d[1] * q.d[1]) + q.d[2] * q.d[2]);
}

// out[0] = loss, out[1] = 1e-3 * mean(angle), out[2] = 0.1 * mean(trn), out[3] = #pairs
__global__ __launch_bounds__(1024) void root_sm1_fwd_kernel(const float* __restrict__ rtk, int stride, int T, const int* __restrict__ off,
                                                            int V, float* __restrict__ out) {
    __shared__ double sh_a[16], sh_t[16];
    __shared__ int sh_c[16];
    double sa = 0.0, st = 0.0;
    int cnt = 0;
    for (int j = threadIdx.x; j < T; j += blockDim.x) {           // j: the first frame of a pair
        int start, end;
        if (!video_of(off, V, T, j, start, end) || j + 1 >= end) continue;
        Pair q;
        pair_eval(rtk, stride, j, q);
        sa += (double)angle_of(q.cosv);
        st += (double)q.trn;
        cnt += 1;
    }
    block_sums<16>(sa, st, cnt, sh_a, sh_t, sh_c);
    if (threadIdx.x == 0) {
        const float rot = (float)(sa / (double)cnt) * 1e-3f;      // no pair: 0 / 0 = NaN, the mean of an empty set
        const float trn = (float)(st / (double)cnt) * 0.1f;
        out[0] = rot + trn;
        out[1] = rot;
        out[2] = trn;
        out[3] = (float)cnt;
    }
}

__global__ __launch_bounds__(256) void root_sm1_bwd_kernel(const float* __restrict__ rtk, int stride, int T, const int* __restrict__ off,
                                                           int V, const float* __restrict__ out, const float* __restrict__ g,
                                                           float* __restrict__ drtk) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= T) return;
    float dR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dt[3] = {0.f, 0.f, 0.f};
    int start, end;
    if (video_of(off, V, T, f, start, end)) {
        const float cnt = out[3];
        const float ca = g[0] * 1e-3f / cnt, ct = g[0] * 0.1f / cnt;
        for (int r = 0; r < 2; ++r) {                              // frame f as the first, then the second frame of a pair
            const int j = f - r;
            if (j < start || j + 1 >= end) continue;
            Pair q;
            pair_eval(rtk, stride, j, q);
            const float gc = ca * dangle_of(q.cosv) * 0.5f;
            const float gt = q.trn > 0.f ? ct / q.trn : 0.f;       // torch's norm backward: 0 at norm 0
            const float sgn = r == 0 ? 1.f : -1.f;
            const float* other = r == 0 ? q.R1 : q.R0;             // cos = <R0, R1> / 2 - 1/2
#pragma unroll
            for (int c = 0; c < 3; ++c) dt[c] += sgn * gt * q.d[c];
#pragma unroll
            for (int i = 0; i < 9; ++i) dR[i] += gc * other[i];
        }
    }
    store_pose_grad(drtk, stride, f, dR, dt);
}

// ---- matrix -> quaternion ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void matrix_to_quat_kernel(const float* __restrict__ R, long long T, long long mat_stride,
                                                             long long row_stride, float* __restrict__ quat) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const float* m = R + i * mat_stride;
    const float r00 = m[0], r01 = m[1], r02 = m[2];
    const float r10 = m[row_stride], r11 = m[row_stride + 1], r12 = m[row_stride + 2];
    const float r20 = m[2 * row_stride], r21 = m[2 * row_stride + 1], r22 = m[2 * row_stride + 2];
    const float d0 = ((1.f + r00) + r11) + r22, d1 = ((1.f + r00) - r11) - r22;
    const float d2 = ((1.f - r00) + r11) - r22, d3 = ((1.f - r00) - r11) + r22;
    int best = 0;                                                  // the largest 4 q_k^2; a tie goes to the lowest index
    float dm = d0;
    if (d1 > dm) { dm = d1; best = 1; }
    if (d2 > dm) { dm = d2; best = 2; }
    if (d3 > dm) { dm = d3; best = 3; }
    float w, x, y, z;                                              // 4 q_best * (q_w, q_x, q_y, q_z)
    if (best == 0) { w = d0; x = r21 - r12; y = r02 - r20; z = r10 - r01; }
    else if (best == 1) { w = r21 - r12; x = d1; y = r01 + r10; z = r02 + r20; }
    else if (best == 2) { w = r02 - r20; x = r01 + r10; y = d2; z = r12 + r21; }
    else { w = r10 - r01; x = r02 + r20; y = r12 + r21; z = d3; }
    const float n = sqrtf(((w * w + x * x) + y * y) + z * z);
    float s = 1.f / n;
    if (w < 0.f) s = -s;                                           // the real part non-negative
    *reinterpret_cast<float4*>(quat + 4 * i) = make_float4(w * s, x * s, y * s, z * s);
}

}  // namespace

extern "C" int moda_shape_target(const float* u, int64_t N, const float* obj_bound, float bound_factor, int32_t ellips, float* pts,
                                 float* dis, void* stream) {
    if (!u || !obj_bound || !pts || !dis || pts == u) return MODA_EINVAL;
    if (N < 1 || 3 * N >= (1LL << 31)) return MODA_ESHAPE;
    hipLaunchKernelGGL(shape_target_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, u, (long long)N, obj_bound,
                       bound_factor, (int)(ellips != 0), pts, dis);
    return (int)hipGetLastError();
}

static int sum_blocks(int64_t N) {
    const long long want = (N + 255) / 256;
    return (int)(want < MODA_SHAPE_LOSS_MAX_BLOCKS ? want : MODA_SHAPE_LOSS_MAX_BLOCKS);
}

extern "C" int moda_shape_loss_fwd(const float* y, const float* dis, int64_t N, double* partials, float* loss, void* stream) {
    if (!y || !dis || !partials || !loss) return MODA_EINVAL;
    if (N < 1 || N >= (1LL << 31)) return MODA_ESHAPE;
    const int nb = sum_blocks(N);
    hipLaunchKernelGGL(sum_partial_kernel<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, y, dis, (long long)N, partials);
    hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)partials, nb, (double)N, loss);
    return (int)hipGetLastError();
}

extern "C" int moda_shape_loss_bwd(const float* y, const float* dis, int64_t N, const float* g, float* dy, double* partials,
                                   float* dy_sum, void* stream) {
    if (!y || !dis || !g || !dy || (dy_sum && !partials)) return MODA_EINVAL;
    if (N < 1 || N >= (1LL << 31)) return MODA_ESHAPE;
    hipLaunchKernelGGL(shape_loss_bwd_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, dis, (long long)N, g, dy);
    if (dy_sum) {
        const int nb = sum_blocks(N);
        hipLaunchKernelGGL(sum_partial_kernel<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const float*)dy,
                           (const float*)nullptr, (long long)N, partials);
        hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const double*)partials, nb, 1.0, dy_sum);
    }
    return (int)hipGetLastError();
}

extern "C" int moda_rtk_loss_fwd(const float* rtk, int32_t rows, const float* rtk_gt, int32_t rows_gt, int64_t T, float* out3,
                                 void* stream) {
    if (!pose_args_ok(rtk, rows, T) || !pose_args_ok(rtk_gt, rows_gt, T) || !out3) return MODA_EINVAL;
    hipLaunchKernelGGL(rtk_loss_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rtk, rows * 4, rtk_gt, rows_gt * 4, (int)T, out3);
    return (int)hipGetLastError();
}

extern "C" int moda_rtk_loss_bwd(const float* rtk, int32_t rows, const float* rtk_gt, int32_t rows_gt, int64_t T, const float* g_total,
                                 const float* g_rot, const float* g_trn, float* drtk, void* stream) {
    if (!pose_args_ok(rtk, rows, T) || !pose_args_ok(rtk_gt, rows_gt, T) || !drtk || !al16(drtk)) return MODA_EINVAL;
    hipLaunchKernelGGL(rtk_loss_bwd_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rtk, rows * 4, rtk_gt,
                       rows_gt * 4, (int)T, g_total, g_rot, g_trn, drtk);
    return (int)hipGetLastError();
}

extern "C" int moda_root_sm1_fwd(const float* rtk, int32_t rows, int64_t T, const int32_t* offsets, int32_t n_videos, float* out4,
                                 void* stream) {
    if (!pose_args_ok(rtk, rows, T) || !offsets || !out4 || n_videos < 1) return MODA_EINVAL;
    hipLaunchKernelGGL(root_sm1_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rtk, rows * 4, (int)T, offsets, (int)n_videos, out4);
    return (int)hipGetLastError();
}

extern "C" int moda_root_sm1_bwd(const float* rtk, int32_t rows, int64_t T, const int32_t* offsets, int32_t n_videos, const float* out4,
                                 const float* g, float* drtk, void* stream) {
    if (!pose_args_ok(rtk, rows, T) || !offsets || !out4 || n_videos < 1 || !g || !drtk || !al16(drtk)) return MODA_EINVAL;
    hipLaunchKernelGGL(root_sm1_bwd_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rtk, rows * 4, (int)T,
                       offsets, (int)n_videos, out4, g, drtk);
    return (int)hipGetLastError();
}

extern "C" int moda_matrix_to_quat(const float* R, int64_t T, int64_t mat_stride, int64_t row_stride, float* quat, void* stream) {
    if (!R || !quat || mat_stride < 0 || row_stride < 3 || !al16(quat)) return MODA_EINVAL;
    if (T < 1 || T >= (1LL << 31)) return MODA_ESHAPE;
    hipLaunchKernelGGL(matrix_to_quat_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, R, (long long)T,
                       (long long)mat_stride, (long long)row_stride, quat);
    return (int)hipGetLastError();
}
