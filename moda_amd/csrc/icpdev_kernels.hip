// The host half of an ICP iteration, on the device (moda_amd/mesh_eval.py: iterative_closest_point_device, eval_sequence): the
// 3 x 3 alignment from the float64 sums of moda_icp_moments, the convergence state, and the per-frame metrics row.  With the
// ragged / masked launches of pointset_kernels.hip an iteration needs no read-back and can be captured into a graph.
//
//   solve     one lane per cloud, float64, nothing contracted.  Means, centred cross-covariance C, then a one-sided (Hestenes)
//             Jacobi SVD: the column pairs (0,1), (0,2), (1,2) of A = C are rotated orthogonal, `sweeps` times round; V collects
//             the rotations.  Then sigma_k = |a_k|, sorted descending (stable), and C = U diag(sigma) V^T with
//             SIGN RULE  sigma_k >= 0; u_0 = a_0 / sigma_0; u_1 = a_1 made orthogonal to u_0 and normalised; u_2 = +-(u_0 x u_1), the
//             sign that of (u_0 x u_1) . a_2 (+ when that is 0).  So U is orthonormal whatever the rank; where a_1 vanishes against
//             a_0 any unit vector orthogonal to u_0 is taken, and C == 0 gives U = V = I (R = I, as LAPACK gives).
//             E = (1, 1, det(U V^T)) unless allow_reflection; R = U E V^T; s = trace(S E) / var(X); T = my - (s mx) R: the
//             arithmetic of mesh_eval._align, rounded once to the fp32 row moda_sim3_apply reads.
//   advance   one workgroup for all clouds: rmse, relative improvement, iteration count, and who goes on.  per_element: a cloud
//             stops when it converges itself; otherwise nobody stops until all have converged in the same iteration (pytorch3d's
//             rule) -- the AND over the clouds is a workgroup vote, and the int32 word it leaves in flags[0] ("someone is still
//             active") is written by one plain vector store; the next launch on the stream reads it.
//   metrics   one workgroup per frame, integer counts and float64 sums over a fixed tree: the same bits on every run.
// Device memory is written only by plain vector stores; no atomics, no device-side assert or print.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kNSum = MODA_ICP_NSUM;
constexpr int kNMetric = MODA_SEQ_NMETRIC;

__device__ __forceinline__ void rotate_pair(double (&A)[3][3], double (&V)[3][3], int p, int q) {
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        alpha += A[i][p] * A[i][p];
        beta += A[i][q] * A[i][q];
        gamma += A[i][p] * A[i][q];
    }
    if (gamma == 0.0) return;                                               // already orthogonal (or a zero column)
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));   // zeta = +-inf: t = 0
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double ap = A[i][p], aq = A[i][q], vp = V[i][p], vq = V[i][q];
        A[i][p] = c * ap - s * aq;
        A[i][q] = s * ap + c * aq;
        V[i][p] = c * vp - s * vq;
        V[i][q] = s * vp + c * vq;
    }
}

__device__ __forceinline__ void swap_cols(double (&A)[3][3], double (&V)[3][3], double (&sg)[3], int p, int q) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double v = A[i][p]; A[i][p] = A[i][q]; A[i][q] = v;
        v = V[i][p]; V[i][p] = V[i][q]; V[i][q] = v;
    }
    const double v = sg[p]; sg[p] = sg[q]; sg[q] = v;
}

__global__ __launch_bounds__(64) void icp_solve_kernel(const double* __restrict__ sums, int B, double n, int estimate_scale,
                                                       int allow_reflection, int sweeps, const int* __restrict__ active,
                                                       float* __restrict__ rts) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B || (active && !active[b])) return;
    const double* q = sums + (int64_t)b * kNSum;
    double mx[3], my[3], A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mx[c] = q[c] / n;
        my[c] = q[3 + c] / n;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) A[c][d] = q[6 + 3 * c + d] / n - mx[c] * my[d];
    for (int s = 0; s < sweeps; ++s) {
        rotate_pair(A, V, 0, 1);
        rotate_pair(A, V, 0, 2);
        rotate_pair(A, V, 1, 2);
    }
    double sg[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) sg[k] = sqrt(A[0][k] * A[0][k] + A[1][k] * A[1][k] + A[2][k] * A[2][k]);
    if (sg[0] < sg[1]) swap_cols(A, V, sg, 0, 1);                           // stable descending order of three
    if (sg[1] < sg[2]) swap_cols(A, V, sg, 1, 2);
    if (sg[0] < sg[1]) swap_cols(A, V, sg, 0, 1);

    double U[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    if (sg[0] > 0.0 && 1.0 / sg[0] < __builtin_huge_val()) {
        double u0[3], u1[3], w[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) u0[i] = A[i][0] / sg[0];
        const double dp = A[0][1] * u0[0] + A[1][1] * u0[1] + A[2][1] * u0[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = A[i][1] - dp * u0[i];
        double r2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
        if (!(r2 > 1e-30 * sg[0] * sg[0])) {                                // a_1 vanishes against a_0: any direction across u_0
            const int k = fabs(u0[0]) <= fabs(u0[1]) ? (fabs(u0[0]) <= fabs(u0[2]) ? 0 : 2) : (fabs(u0[1]) <= fabs(u0[2]) ? 1 : 2);
#pragma unroll
            for (int i = 0; i < 3; ++i) w[i] = (i == k ? 1.0 : 0.0) - u0[k] * u0[i];
            r2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
        }
        const double g = 1.0 / sqrt(r2);
#pragma unroll
        for (int i = 0; i < 3; ++i) u1[i] = w[i] * g;
        double u2[3] = {u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]};
        const double side = u2[0] * A[0][2] + u2[1] * A[1][2] + u2[2] * A[2][2];
        const double sgn = side < 0.0 ? -1.0 : 1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            U[i][0] = u0[i];
            U[i][1] = u1[i];
            U[i][2] = sgn * u2[i];
        }
    }
    double E[3] = {1.0, 1.0, 1.0};
    if (!allow_reflection) {
        double Mt[3][3];                                                    // U V^T
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) Mt[i][j] = U[i][0] * V[j][0] + U[i][1] * V[j][1] + U[i][2] * V[j][2];
        E[2] = Mt[0][0] * (Mt[1][1] * Mt[2][2] - Mt[1][2] * Mt[2][1]) - Mt[0][1] * (Mt[1][0] * Mt[2][2] - Mt[1][2] * Mt[2][0])
             + Mt[0][2] * (Mt[1][0] * Mt[2][1] - Mt[1][1] * Mt[2][0]);
    }
    double R[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = U[i][0] * E[0] * V[j][0] + U[i][1] * E[1] * V[j][1] + U[i][2] * E[2] * V[j][2];
    double s = 1.0;
    if (estimate_scale) {
        const double var = q[15] / n - (mx[0] * mx[0] + mx[1] * mx[1] + mx[2] * mx[2]);
        s = (sg[0] * E[0] + sg[1] * E[1] + sg[2] * E[2]) / var;
    }
    float* o = rts + (int64_t)b * 13;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (float)R[i][j];
#pragma unroll
    for (int j = 0; j < 3; ++j)
        o[9 + j] = (float)(my[j] - ((s * mx[0]) * R[0][j] + (s * mx[1]) * R[1][j] + (s * mx[2]) * R[2][j]));
    o[12] = (float)s;
}

__global__ __launch_bounds__(kBlock) void icp_advance_kernel(const double* __restrict__ sums, int B, double n, double thr,
                                                             int per_element, double* __restrict__ prev_rmse,
                                                             float* __restrict__ rmse, int* __restrict__ iterations,
                                                             int* __restrict__ converged, int* __restrict__ active,
                                                             int* __restrict__ flags) {
    // pass 1: every active cloud's own verdict; the vote is over the clouds that took part in this iteration
    int all_conv = 1, any_left = 0;
    for (int b = threadIdx.x; b < B; b += kBlock) {
        if (!active[b]) continue;
        const double r = sqrt(sums[(int64_t)b * kNSum + 16] / n), p = prev_rmse[b];
        const int it = iterations[b];
        const double rel = it == 0 ? 1.0 : (p > 0.0 ? (p - r) / p : 0.0);   // an rmse that was already exactly 0: converged
        const int conv = rel <= thr ? 1 : 0;
        prev_rmse[b] = r;
        rmse[b] = (float)r;
        iterations[b] = it + 1;
        if (per_element) {
            converged[b] = conv;
            active[b] = conv ? 0 : 1;
            any_left |= !conv;
        } else {
            all_conv &= conv;
        }
    }
    if (per_element) {
        any_left = __syncthreads_or(any_left);
    } else {
        all_conv = __syncthreads_and(all_conv);                             // the device-wide AND: one workgroup sees every cloud
        for (int b = threadIdx.x; b < B; b += kBlock) {
            if (!active[b]) continue;
            any_left |= !all_conv;
            converged[b] = all_conv;
            active[b] = all_conv ? 0 : 1;
        }
        any_left = __syncthreads_or(any_left);
    }
    if (threadIdx.x == 0) flags[0] = any_left;
}

// row: cd, f001, f002, f005, then (precision_1, precision_2) at each of the three thresholds
__global__ __launch_bounds__(kBlock) void seq_metrics_kernel(const float* __restrict__ d1, const float* __restrict__ d2, int M_max,
                                                             int N, const int* __restrict__ y_len,
                                                             const float* __restrict__ bbox_max, double* __restrict__ out) {
    __shared__ double lds_s[kBlock / 64][2];
    __shared__ int lds_c[kBlock / 64][6];
    const int b = blockIdx.x;
    const int len = min(max(y_len ? y_len[b] : M_max, 0), M_max);
    const double box = (double)bbox_max[b];
    const double fr[3] = {0.01, 0.02, 0.05};
    float thr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v = box * fr[k];
        thr[k] = (float)(v * v);                                            // the fp32 scalar a fp32 tensor is compared with
    }
    double s1 = 0.0, s2 = 0.0;
    int c[6] = {0, 0, 0, 0, 0, 0};
    const float* p1 = d1 + (int64_t)b * M_max;
    const float* p2 = d2 + (int64_t)b * N;
    for (int i = threadIdx.x; i < len; i += kBlock) {
        const float d = p1[i];
        s1 += (double)__fsqrt_rn(d);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[2 * k] += d < thr[k] ? 1 : 0;
    }
    for (int i = threadIdx.x; i < N; i += kBlock) {
        const float d = p2[i];
        s2 += (double)__fsqrt_rn(d);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[2 * k + 1] += d < thr[k] ? 1 : 0;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    s1 = wave_add_down(s1);
    s2 = wave_add_down(s2);
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = wave_add_down(c[k]);
    if (lane == 0) {
        lds_s[w][0] = s1;
        lds_s[w][1] = s2;
#pragma unroll
        for (int k = 0; k < 6; ++k) lds_c[w][k] = c[k];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    s1 = s2 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = 0;
    for (int v = 0; v < kBlock / 64; ++v) {
        s1 += lds_s[v][0];
        s2 += lds_s[v][1];
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] += lds_c[v][k];
    }
    double* o = out + (int64_t)b * kNMetric;
    o[0] = s1 / (double)len + s2 / (double)N;
    const float n1 = (float)len, n2 = (float)N;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // fscore's rule: every quotient formed in float64 from fp32 operands and rounded once to fp32
        const float pa = (float)((double)(float)c[2 * k] / (double)n1), pb = (float)((double)(float)c[2 * k + 1] / (double)n2);
        const float num = 2.0f * pa * pb, den = pa + pb;
        const float f = den == 0.0f ? 0.0f : (float)((double)num / (double)den);      // 0 / 0 is 0
        o[1 + k] = (double)f;
        o[4 + 2 * k] = (double)pa;
        o[5 + 2 * k] = (double)pb;
    }
}

}   // namespace

extern "C" int moda_icp_solve(const double* sums, int64_t B, int64_t N, int32_t estimate_scale, int32_t allow_reflection,
                              int32_t sweeps, const int32_t* active, float* rts, void* stream) {
    if (B < 1 || B >= 2147483648LL || N < 1) return MODA_ESHAPE;
    if (sweeps < 0 || sweeps > 64) return MODA_EINVAL;
    if (!sums || !rts) return MODA_EINVAL;
    hipLaunchKernelGGL(icp_solve_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, sums, (int)B, (double)N,
                       estimate_scale ? 1 : 0, allow_reflection ? 1 : 0, sweeps ? sweeps : MODA_ICP_SOLVE_SWEEPS, active, rts);
    return (int)hipGetLastError();
}

extern "C" int moda_icp_advance(const double* sums, int64_t B, int64_t N, double relative_rmse_thr, int32_t per_element,
                                double* prev_rmse, float* rmse, int32_t* iterations, int32_t* converged, int32_t* active,
                                int32_t* flags, void* stream) {
    if (B < 1 || B >= 2147483648LL || N < 1) return MODA_ESHAPE;
    if (!sums || !prev_rmse || !rmse || !iterations || !converged || !active || !flags) return MODA_EINVAL;
    hipLaunchKernelGGL(icp_advance_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, sums, (int)B, (double)N, relative_rmse_thr,
                       per_element ? 1 : 0, prev_rmse, rmse, iterations, converged, active, flags);
    return (int)hipGetLastError();
}

extern "C" int moda_seq_metrics(const float* dist_gt, const float* dist_pred, int64_t B, int64_t M_max, int64_t N,
                                const int32_t* y_len, const float* bbox_max, double* out, void* stream) {
    if (B < 1 || M_max < 1 || N < 1 || (double)B * (double)M_max >= 2147483648.0 || (double)B * (double)N >= 2147483648.0)
        return MODA_ESHAPE;
    if (!dist_gt || !dist_pred || !bbox_max || !out) return MODA_EINVAL;
    hipLaunchKernelGGL(seq_metrics_kernel, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, dist_gt, dist_pred, (int)M_max,
                       (int)N, y_len, bbox_max, out);
    return (int)hipGetLastError();
}
