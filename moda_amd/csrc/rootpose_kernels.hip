// Root (camera) poses on the device: the tail of RTHead / RTExplicit / RTExpMLP (reference nnutils/nerf.py:307-344, 382-470)
// composed with refine_rt / create_base_se3 and the intrinsics row of convert_root_pose (nnutils/moda.py:1025-1033, 1419-1466),
// the deterministic sum of per-row gradients into a per-frame table, and prepare_ray_cams (moda.py:1036-1046 over
// geom_utils.py:596-652).  One thread per row, fp32, forward and hand-derived backward in one kernel each (g == NULL selects
// forward).  Nothing allocates, synchronises or reads back; no float atomics (the only atomic is the integer count of refused
// ids); floating-point contraction is off for the whole file, so the results are the same bits on every run.
//
// so3_exp restates pytorch3d's so3_exponential_map (absent from the reference tree and unpinned): nrm = sum(w * w),
// theta = sqrt(max(nrm, 1e-4)), R = f1 hat(w) + f2 hat(w)^2 + I with f1 = sin(theta) / theta, f2 = (1 - cos(theta)) / theta^2.
// Below the clamp theta is the constant 0.01 and carries no gradient.  f2 is evaluated as 2 sin^2(theta / 2) / theta^2 and the
// derivatives of f1 and f2 by their series below theta = 0.5: the same functions without the cancellation of the textbook forms.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kIdTile = 1024;

DEVINL void mat_mul(const float* A, const float* B, float* C) {          // C = A B
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
}
DEVINL void mat_tmul(const float* A, const float* B, float* C) {         // C = A^T B
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[r * 3 + c] = A[r] * B[c] + A[3 + r] * B[3 + c] + A[6 + r] * B[6 + c];
}
DEVINL void mat_mult(const float* A, const float* B, float* C) {         // C = A B^T
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[r * 3 + c] = A[r * 3] * B[c * 3] + A[r * 3 + 1] * B[c * 3 + 1] + A[r * 3 + 2] * B[c * 3 + 2];
}
DEVINL void mat_vec(const float* A, const float* v, float* o) {          // o = A v
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = A[r * 3] * v[0] + A[r * 3 + 1] * v[1] + A[r * 3 + 2] * v[2];
}
DEVINL void mat_tvec(const float* A, const float* v, float* o) {         // o = A^T v
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = A[r] * v[0] + A[3 + r] * v[1] + A[6 + r] * v[2];
}

DEVINL void hat(const float* w, float* K) {
    K[0] = 0.f; K[1] = -w[2]; K[2] = w[1];
    K[3] = w[2]; K[4] = 0.f; K[5] = -w[0];
    K[6] = -w[1]; K[7] = w[0]; K[8] = 0.f;
}

DEVINL void so3_exp(const float* w, float* R) {
    const float nrm = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const float theta = sqrtf(fmaxf(nrm, 1e-4f));
    const float sh = sinf(0.5f * theta);
    const float f1 = sinf(theta) / theta, f2 = 2.f * sh * sh / (theta * theta);
    float K[9], K2[9];
    hat(w, K);
    mat_mul(K, K, K2);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = f1 * K[k] + f2 * K2[k] + ((k & 3) == 0 ? 1.f : 0.f);
}

// dL/dw of R = so3_exp(w) given G = dL/dR
DEVINL void so3_exp_bwd(const float* w, const float* G, float* dw) {
    const float nrm = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const float theta = sqrtf(fmaxf(nrm, 1e-4f));
    const float sn = sinf(theta), cs = cosf(theta), sh = sinf(0.5f * theta);
    const float f1 = sn / theta, f2 = 2.f * sh * sh / (theta * theta);
    float K[9], K2[9], GK[9], KG[9];
    hat(w, K);
    mat_mul(K, K, K2);
    mat_mul(G, K, GK);
    mat_mul(K, G, KG);
    float s1 = 0.f, s2 = 0.f, D[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        s1 += G[k] * K[k];
        s2 += G[k] * K2[k];
        D[k] = f1 * G[k] - f2 * (GK[k] + KG[k]);          // dL/dK: K^T = -K
    }
    dw[0] = D[7] - D[5];
    dw[1] = D[2] - D[6];
    dw[2] = D[3] - D[1];
    if (nrm >= 1e-4f) {                                   // torch's clamp passes the gradient AT its bound
        float df1, df2;
        const float t2 = theta * theta;
        if (theta < 0.5f) {
            df1 = theta * (-1.f / 3.f + t2 * (1.f / 30.f + t2 * (-1.f / 840.f + t2 * (1.f / 45360.f))));
            df2 = theta * (-1.f / 12.f + t2 * (1.f / 180.f + t2 * (-1.f / 6720.f + t2 * (1.f / 453600.f))));
        } else {
            df1 = (theta * cs - sn) / t2;
            df2 = (theta * sn - 4.f * sh * sh) / (t2 * theta);
        }
        const float coef = (s1 * df1 + s2 * df2) / theta;
        dw[0] += coef * w[0]; dw[1] += coef * w[1]; dw[2] += coef * w[2];
    }
}

// quaternion_to_matrix(F.normalize(q)): u = q / max(|q|, 1e-12), R = matrix(u) scaled by 2 / |u|^2
DEVINL void quat_exp(const float* q, float* R) {
    const float nrm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float den = fmaxf(nrm, 1e-12f);
    const float r = q[0] / den, i = q[1] / den, j = q[2] / den, k = q[3] / den;
    const float ts = 2.f / (r * r + i * i + j * j + k * k);
    R[0] = 1.f - ts * (j * j + k * k);
    R[1] = ts * (i * j - k * r);
    R[2] = ts * (i * k + j * r);
    R[3] = ts * (i * j + k * r);
    R[4] = 1.f - ts * (i * i + k * k);
    R[5] = ts * (j * k - i * r);
    R[6] = ts * (i * k - j * r);
    R[7] = ts * (j * k + i * r);
    R[8] = 1.f - ts * (i * i + j * j);
}

DEVINL void quat_exp_bwd(const float* q, const float* g, float* dq) {
    const float nrm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float den = fmaxf(nrm, 1e-12f);
    const float r = q[0] / den, i = q[1] / den, j = q[2] / den, k = q[3] / den;
    const float ts = 2.f / (r * r + i * i + j * j + k * k);
    const float Gs = -g[0] * (j * j + k * k) + g[1] * (i * j - k * r) + g[2] * (i * k + j * r) + g[3] * (i * j + k * r)
                     - g[4] * (i * i + k * k) + g[5] * (j * k - i * r) + g[6] * (i * k - j * r) + g[7] * (j * k + i * r)
                     - g[8] * (i * i + j * j);
    float a[4];
    a[0] = -k * g[1] + j * g[2] + k * g[3] - i * g[5] - j * g[6] + i * g[7];
    a[1] = j * g[1] + k * g[2] + j * g[3] - 2.f * i * g[4] - r * g[5] + k * g[6] + r * g[7] - 2.f * i * g[8];
    a[2] = -2.f * j * g[0] + i * g[1] + r * g[2] + i * g[3] + k * g[5] - r * g[6] + k * g[7] - 2.f * j * g[8];
    a[3] = -2.f * k * g[0] - r * g[1] + i * g[2] + r * g[3] - 2.f * k * g[4] + j * g[5] + i * g[6] + j * g[7];
    const float c = ts * ts * Gs;
    const float u[4] = {r, i, j, k};
    float du[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) du[m] = ts * a[m] - c * u[m];
    if (nrm >= 1e-12f) {
        const float dot = du[0] * u[0] + du[1] * u[1] + du[2] * u[2] + du[3] * u[3];
#pragma unroll
        for (int m = 0; m < 4; ++m) dq[m] = (du[m] - u[m] * dot) / den;
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) dq[m] = du[m] / den;
    }
}

// one head row [t (3) | rotation (cols - 3)] -> (R, t): 7 columns a quaternion, 6 a rotation vector; t = 0.1 * row[0:3]
DEVINL void head_fwd(const float* row, int cols, float* R, float* t) {
    t[0] = row[0] * 0.1f; t[1] = row[1] * 0.1f; t[2] = row[2] * 0.1f;
    if (cols == 7) quat_exp(row + 3, R);
    else so3_exp(row + 3, R);
}
DEVINL void head_bwd(const float* row, int cols, const float* gR, const float* gt, float scale, float* d) {
    float gs[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) gs[k] = gR[k] * scale;
    d[0] = gt[0] * scale * 0.1f; d[1] = gt[1] * scale * 0.1f; d[2] = gt[2] * scale * 0.1f;
    if (cols == 7) quat_exp_bwd(row + 3, gs, d + 3);
    else so3_exp_bwd(row + 3, gs, d + 3);
}

__global__ void root_pose_kernel(const float* __restrict__ se3, long long T, int cols, const void* __restrict__ ids, int ids64,
                                 long long n, const float* __restrict__ delta, int dcols, const float* __restrict__ rt_raw,
                                 int raw_mode, int raw_ld, float obj_scale, const float* __restrict__ ks,
                                 const void* __restrict__ dataid, int dataid64, long long n_ks, int out_rows,
                                 float* __restrict__ rtk, const float* __restrict__ g, float* __restrict__ d_rows,
                                 float* __restrict__ d_delta, float* __restrict__ d_ks_rows, int* __restrict__ status) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool fwd = g == nullptr;
    const int ld = out_rows * 4;
    const float nan = __builtin_nanf("");
    long long id = 0;
    if (se3 != nullptr || raw_mode == MODA_ROOT_RAW_BY_ID) {
        id = load_id(ids, ids64, i);
        if (id < 0 || id >= T) {                           // refused: counted once (forward), nothing is read through it
            if (fwd) {
                atomicAdd(status, 1);
                for (int k = 0; k < ld; ++k) rtk[i * ld + k] = nan;
            } else {
                if (d_rows) for (int k = 0; k < cols; ++k) d_rows[i * cols + k] = 0.f;
                if (d_delta) for (int k = 0; k < dcols; ++k) d_delta[i * dcols + k] = 0.f;
                if (d_ks_rows) for (int k = 0; k < 4; ++k) d_ks_rows[i * 4 + k] = 0.f;
            }
            return;
        }
    }
    // ---- forward values (recomputed by the backward) ----
    float Rb[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tb[3] = {0.f, 0.f, 0.f};
    float Rd[9], td[3], Rr[9], tr[3], R0[9], t0[3];
    float brow[7], drow[7];
    const bool both = se3 != nullptr && delta != nullptr;
    if (se3) {
        for (int k = 0; k < cols; ++k) brow[k] = se3[id * cols + k];
        head_fwd(brow, cols, Rb, tb);
        if (both) {                                        // nerf.py:456: x * 10 - (x * 9).detach(), two roundings and a difference
#pragma unroll
            for (int k = 0; k < 9; ++k) Rb[k] = Rb[k] * 10.f - Rb[k] * 9.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) tb[k] = tb[k] * 10.f - tb[k] * 9.f;
        }
    }
    if (delta) {
        for (int k = 0; k < dcols; ++k) drow[k] = delta[i * dcols + k];
        head_fwd(drow, dcols, Rd, td);
    }
    if (both) {                                            // nerf.py:464-465
        float v[3];
        mat_vec(Rb, td, v);
        tr[0] = tb[0] + v[0]; tr[1] = tb[1] + v[1]; tr[2] = tb[2] + v[2];
        mat_mul(Rb, Rd, Rr);
    } else {
        const float* Rs = delta ? Rd : Rb;
        const float* ts = delta ? td : tb;
#pragma unroll
        for (int k = 0; k < 9; ++k) Rr[k] = Rs[k];
        tr[0] = ts[0]; tr[1] = ts[1]; tr[2] = ts[2];
    }
    const bool has_raw = raw_mode == MODA_ROOT_RAW_ROWS || raw_mode == MODA_ROOT_RAW_BY_ID;
    if (has_raw) {
        const float* p = rt_raw + (raw_mode == MODA_ROOT_RAW_BY_ID ? id : i) * raw_ld;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            R0[r * 3] = p[r * 4]; R0[r * 3 + 1] = p[r * 4 + 1]; R0[r * 3 + 2] = p[r * 4 + 2];
            t0[r] = p[r * 4 + 3] / obj_scale;
        }
    }
    if (fwd) {
        float R[9], t[3];
        if (has_raw) {                                     // moda.py:1460-1463
            float v[3];
            mat_vec(R0, tr, v);
            t[0] = t0[0] + v[0]; t[1] = t0[1] + v[1]; t[2] = t0[2] + v[2];
            mat_mul(R0, Rr, R);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = Rr[k];
            t[0] = tr[0]; t[1] = tr[1]; t[2] = tr[2];
            if (raw_mode == MODA_ROOT_RAW_BASE) t[2] = 0.3f + tr[2];     // create_base_se3: identity, (0, 0, 0.3)
        }
        float* o = rtk + i * ld;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            o[r * 4] = R[r * 3]; o[r * 4 + 1] = R[r * 3 + 1]; o[r * 4 + 2] = R[r * 3 + 2]; o[r * 4 + 3] = t[r];
        }
        if (out_rows == 4) {
            float k4[4] = {0.f, 0.f, 0.f, 1.f};
            if (ks) {
                const long long v = load_id(dataid, dataid64, i);
                if (v < 0 || v >= n_ks) {
                    atomicAdd(status + 1, 1);
                    k4[0] = k4[1] = k4[2] = k4[3] = nan;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) k4[k] = ks[v * 4 + k];
                }
            }
            o[12] = k4[0]; o[13] = k4[1]; o[14] = k4[2]; o[15] = k4[3];
        }
        return;
    }
    // ---- backward ----
    const float* gi = g + i * ld;
    float gR[9], gt[3], gRr[9], gtr[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        gR[r * 3] = gi[r * 4]; gR[r * 3 + 1] = gi[r * 4 + 1]; gR[r * 3 + 2] = gi[r * 4 + 2]; gt[r] = gi[r * 4 + 3];
    }
    if (d_ks_rows) {
        bool ok = out_rows == 4 && ks != nullptr;
        if (ok) {
            const long long v = load_id(dataid, dataid64, i);
            ok = v >= 0 && v < n_ks;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) d_ks_rows[i * 4 + k] = ok ? gi[12 + k] : 0.f;
    }
    if (has_raw) {
        mat_tmul(R0, gR, gRr);
        mat_tvec(R0, gt, gtr);
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) gRr[k] = gR[k];
        gtr[0] = gt[0]; gtr[1] = gt[1]; gtr[2] = gt[2];
    }
    if (both) {
        float gRb[9], gRd[9], gtd[3], dout[7];
        mat_mult(gRr, Rd, gRb);                            // R = Rb Rd
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) gRb[r * 3 + c] += gtr[r] * td[c];     // t = tb + Rb td
        mat_tmul(Rb, gRr, gRd);
        mat_tvec(Rb, gtr, gtd);
        head_bwd(brow, cols, gRb, gtr, 10.f, dout);        // the magnified gradient of nerf.py:456
        for (int k = 0; k < cols; ++k) d_rows[i * cols + k] = dout[k];
        head_bwd(drow, dcols, gRd, gtd, 1.f, dout);
        for (int k = 0; k < dcols; ++k) d_delta[i * dcols + k] = dout[k];
    } else if (se3) {
        float dout[7];
        head_bwd(brow, cols, gRr, gtr, 1.f, dout);
        for (int k = 0; k < cols; ++k) d_rows[i * cols + k] = dout[k];
    } else if (delta) {
        float dout[7];
        head_bwd(drow, dcols, gRr, gtr, 1.f, dout);
        for (int k = 0; k < dcols; ++k) d_delta[i * dcols + k] = dout[k];
    }
}

// d_table (T, C) = sum of rows[i] over ids[i] == t, added in increasing i: one lane per table row, the ids staged through LDS in
// tiles of kIdTile and read by every lane at once (a broadcast).  The order of the additions does not depend on the launch shape.
__global__ void id_rows_sum_kernel(const float* __restrict__ rows, const void* __restrict__ ids, int ids64, long long n, long long T,
                                   int C, float* __restrict__ d_table) {
    __shared__ int sh[kIdTile];
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    float acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
    for (long long base = 0; base < n; base += kIdTile) {
        const int m = (int)((n - base) < (long long)kIdTile ? (n - base) : (long long)kIdTile);
        __syncthreads();
        for (int j = threadIdx.x; j < m; j += blockDim.x) {
            const long long v = load_id(ids, ids64, base + j);
            sh[j] = (v >= 0 && v < T) ? (int)v : -1;
        }
        __syncthreads();
        if (t < T) {
            for (int j = 0; j < m; ++j) {
                if (sh[j] == (int)t) {
                    const float* r = rows + (base + j) * C;
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        if (c < C) acc[c] += r[c];
                }
            }
        }
    }
    if (t < T) {
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c < C) d_table[t * C + c] = acc[c];
    }
}

// prepare_ray_cams (moda.py:1036-1046): Kinv = Kmatinv(K2inv(kaug) @ K2mat(rtk[:, 3])), the reference's quotient forms
__global__ void ray_cams_kernel(const float* __restrict__ rtk, const float* __restrict__ kaug, long long n, float* __restrict__ Rmat,
                                float* __restrict__ Tmat, float* __restrict__ Kinv, const float* __restrict__ g_R,
                                const float* __restrict__ g_T, const float* __restrict__ g_K, float* __restrict__ d_rtk, int bwd) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = rtk + i * 16;
    const float fx = p[12], fy = p[13], px = p[14], py = p[15];
    const float ax = kaug[i * 4], ay = kaug[i * 4 + 1], apx = kaug[i * 4 + 2], apy = kaug[i * 4 + 3];
    const float ix = 1.f / ax, iy = 1.f / ay;
    const float P00 = ix * fx, P11 = iy * fy;              // (Kaug Kmat): the zero products of the 3x3 product add nothing
    const float P02 = ix * px + (-apx / ax), P12 = iy * py + (-apy / ay);
    if (!bwd) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            Rmat[i * 9 + r * 3] = p[r * 4]; Rmat[i * 9 + r * 3 + 1] = p[r * 4 + 1]; Rmat[i * 9 + r * 3 + 2] = p[r * 4 + 2];
            Tmat[i * 3 + r] = p[r * 4 + 3];
        }
        float* o = Kinv + i * 9;
        o[0] = 1.f / P00; o[1] = 0.f; o[2] = -P02 / P00;
        o[3] = 0.f; o[4] = 1.f / P11; o[5] = -P12 / P11;
        o[6] = 0.f; o[7] = 0.f; o[8] = 1.f;
        return;
    }
    float* d = d_rtk + i * 16;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        d[r * 4] = g_R ? g_R[i * 9 + r * 3] : 0.f;
        d[r * 4 + 1] = g_R ? g_R[i * 9 + r * 3 + 1] : 0.f;
        d[r * 4 + 2] = g_R ? g_R[i * 9 + r * 3 + 2] : 0.f;
        d[r * 4 + 3] = g_T ? g_T[i * 3 + r] : 0.f;
    }
    float dfx = 0.f, dfy = 0.f, dpx = 0.f, dpy = 0.f;
    if (g_K) {
        const float g00 = g_K[i * 9], g02 = g_K[i * 9 + 2], g11 = g_K[i * 9 + 4], g12 = g_K[i * 9 + 5];
        const float dP00 = (g02 * P02 - g00) / (P00 * P00), dP02 = -g02 / P00;
        const float dP11 = (g12 * P12 - g11) / (P11 * P11), dP12 = -g12 / P11;
        dfx = dP00 * ix; dpx = dP02 * ix;
        dfy = dP11 * iy; dpy = dP12 * iy;
    }
    d[12] = dfx; d[13] = dfy; d[14] = dpx; d[15] = dpy;
}

}   // namespace

extern "C" int moda_root_pose(const float* se3, int64_t T, int32_t cols, const void* ids, int32_t ids64, int64_t n,
                              const float* delta, int32_t delta_cols, const float* rt_raw, int32_t raw_mode, int32_t raw_rows,
                              float obj_scale, const float* ks, const void* dataid, int32_t dataid64, int64_t n_ks,
                              int32_t out_rows, float* rtk, const float* g_rtk, float* d_rows, float* d_delta, float* d_ks_rows,
                              int32_t* status, void* stream) {
    if (n <= 0) return 0;
    if (n > 0x7fffffffLL * kBlock || (out_rows != 3 && out_rows != 4) || !status) return MODA_EINVAL;
    if (se3 && ((cols != 6 && cols != 7) || T < 1 || !ids)) return MODA_EINVAL;
    if (delta && delta_cols != 6 && delta_cols != 7) return MODA_EINVAL;
    if (raw_mode < MODA_ROOT_RAW_NONE || raw_mode > MODA_ROOT_RAW_BY_ID) return MODA_EINVAL;
    if (raw_mode >= MODA_ROOT_RAW_ROWS && (!rt_raw || (raw_rows != 3 && raw_rows != 4) || !(obj_scale > 0.f))) return MODA_EINVAL;
    if (raw_mode == MODA_ROOT_RAW_BY_ID && (!ids || T < 1)) return MODA_EINVAL;
    if (ks && (!dataid || n_ks < 1 || out_rows != 4)) return MODA_EINVAL;
    if (g_rtk ? ((se3 && !d_rows) || (delta && !d_delta)) : !rtk) return MODA_EINVAL;
    hipLaunchKernelGGL(root_pose_kernel, dim3(nblocks(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, se3, (long long)T, (int)cols,
                       ids, (int)ids64, (long long)n, delta, (int)delta_cols, rt_raw, (int)raw_mode, (int)raw_rows * 4, obj_scale, ks,
                       dataid, (int)dataid64, (long long)n_ks, (int)out_rows, rtk, g_rtk, d_rows, d_delta, d_ks_rows, (int*)status);
    return (int)hipGetLastError();
}

extern "C" int moda_id_rows_sum(const float* rows, const void* ids, int32_t ids64, int64_t n, int64_t T, int32_t C, float* d_table,
                                int32_t lanes, void* stream) {
    if (T <= 0) return 0;
    if (n < 0 || T > 0x7fffffffLL || C < 1 || C > 8 || !d_table || (n > 0 && (!rows || !ids))) return MODA_EINVAL;
    const int block = lanes == 0 ? kBlock : lanes;
    if (block < 64 || block > 1024 || block % 64) return MODA_EINVAL;
    hipLaunchKernelGGL(id_rows_sum_kernel, dim3(nblocks(T, block)), dim3(block), 0, (hipStream_t)stream, rows, ids, (int)ids64,
                       (long long)n, (long long)T, (int)C, d_table);
    return (int)hipGetLastError();
}

extern "C" int moda_ray_cams(const float* rtk, const float* kaug, int64_t n, float* Rmat, float* Tmat, float* Kinv, const float* g_Rmat,
                             const float* g_Tmat, const float* g_Kinv, float* d_rtk, void* stream) {
    if (n <= 0) return 0;
    if (!rtk || !kaug || n > 0x7fffffffLL * kBlock) return MODA_EINVAL;
    const int bwd = d_rtk != nullptr;
    if (!bwd && (!Rmat || !Tmat || !Kinv)) return MODA_EINVAL;
    hipLaunchKernelGGL(ray_cams_kernel, dim3(nblocks(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, rtk, kaug, (long long)n, Rmat,
                       Tmat, Kinv, g_Rmat, g_Tmat, g_Kinv, d_rtk, bwd);
    return (int)hipGetLastError();
}
