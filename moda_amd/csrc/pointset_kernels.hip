// Point-set kernels for mesh evaluation (reference scripts/visualize/render_vis.py:379-417): the nearest-neighbour search
// behind Chamfer distance and ICP (third_party/chamfer3D/chamfer3D.cu:12-134 NmDistanceKernel, pytorch3d knn_points K = 1),
// the Chamfer gradient (chamfer3D.cu:155-174) and the sums an ICP step needs.  VALU-bound: no MFMA (the distance is formed
// from fp32 differences, not from the |x|^2 + |y|^2 - 2 x.y expansion a matrix product would compute).
//
//   nn          brute force.  A 256-thread workgroup owns 1024 queries, four per lane in registers as two packed pairs
//               (v_pk_add / v_pk_mul / v_pk_fma_f32: two queries per instruction).  Targets pass through LDS in tiles of 1024,
//               stored as three planes (x, y, z); every lane reads the SAME four targets with one 16-byte read per plane (a
//               uniform address: a broadcast, no bank conflict), so three LDS reads feed 16 distance evaluations per lane.
//               Per query and group of four targets the group minimum is compared (strict <) with the running best and only
//               the group's base index is kept; after the scan the winning group is evaluated once more from global memory
//               and the first target whose distance equals the best is the answer: lowest index among equal distances,
//               as the reference's in-order scan with a strict < gives.
//   distance    d = fma(dz, dz, fma(dy, dy, dx * dx)) with dx = qx - tx etc., every operation rounded on its own in fp32
//               (contraction is switched off for this file and the two FMAs are written out, so the packed scan and the
//               scalar re-evaluation produce the same bits).
//   split       when B * ceil(N / 1024) workgroups would leave CUs idle the targets are also split into ranges.  Each
//               range's result is a 64-bit key (bits(d) << 32) | idx -- d >= 0, so its bits order as an unsigned integer --
//               combined with atomicMin: minimum distance, then lowest index, whatever order the workgroups finish in.
//   moments     per-thread float64 sums, a fixed shuffle / LDS tree per workgroup, partials added in index order by a second
//               kernel: no float atomics, the same bits on every run.
//   ragged      moda_nn_fwd_ragged / moda_icp_moments_ragged / moda_sim3_apply_masked run the SAME kernels with two more pointers:
//               y_len[b] (only y[b, :y_len[b]] are targets: the tile load stops there, so padding rows are never read as
//               candidates, whatever they hold) and active[b] (0: every workgroup of cloud b returns before it touches LDS or
//               a barrier, and that cloud's outputs keep their bits).  The dense entries pass NULL for both.
// Device memory is written only by plain vector stores and HIP atomic functions.  Indices are int32 (the entry points refuse
// B * N or B * M >= 2^31); element offsets are formed in 64 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int kBlock = 256;
constexpr int kQ = 4;                      // queries per lane
constexpr int kQB = kBlock * kQ;           // MODA_NN_QUERY_BLOCK
constexpr int kTile = 1024;                // MODA_NN_TILE: targets per LDS tile, 3 planes x 4 KB
constexpr int kGroup = 4;                  // targets per LDS read and per index update
constexpr int kTargetBlocks = 1024;        // four workgroups per CU on 256 CUs
constexpr int kNSum = MODA_ICP_NSUM;
constexpr int kIcpMaxBlocks = MODA_ICP_MAX_BLOCKS;

DEVINL f2 dist2_pk(f2 qx, f2 qy, f2 qz, float tx, float ty, float tz) {
    const f2 dx = qx - tx, dy = qy - ty, dz = qz - tz;
    f2 d = dx * dx;
    d = __builtin_elementwise_fma(dy, dy, d);
    return __builtin_elementwise_fma(dz, dz, d);
}

DEVINL float dist2_1(float qx, float qy, float qz, float tx, float ty, float tz) {
    const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
    float d = dx * dx;
    d = __builtin_fmaf(dy, dy, d);
    return __builtin_fmaf(dz, dz, d);
}

// splits > 1: results go to keys through atomicMin; splits == 1: dist2 / idx are written directly
__global__ __launch_bounds__(kBlock) void nn_kernel(const float* __restrict__ x, const float* __restrict__ y, int N, int M,
                                                    int nblk, int splits, int range, const int* __restrict__ y_len,
                                                    const int* __restrict__ active, float* __restrict__ dist2,
                                                    int* __restrict__ idx, unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) float lds[3][kTile];
    const int t = threadIdx.x;
    const int per_b = nblk * splits;
    const int b = blockIdx.x / per_b, r = blockIdx.x - b * per_b;
    if (active && !active[b]) return;                                       // a skipped cloud: before any LDS access or barrier
    const int s = r / nblk, qb = r - s * nblk;
    // dense: the host makes every range non-empty.  ragged: y has M rows per cloud of which the first y_len[b] are targets; a
    // range that begins past them has no candidate and leaves its keys alone (block-uniform, before the first barrier)
    const int len = y_len ? min(y_len[b], M) : M;
    const int m_begin = s * range, m_end = min(len, m_begin + range);
    if (m_begin >= m_end) return;
    const float* xb = x + (int64_t)b * N * 3;
    const float* yb = y + (int64_t)b * M * 3;
    const int q0 = qb * kQB + t;

    float qx[kQ], qy[kQ], qz[kQ], best[kQ];
    int bj[kQ];
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        const int i = min(q0 + k * kBlock, N - 1);                          // lanes past N repeat the last query; not stored
        qx[k] = xb[(int64_t)i * 3 + 0];
        qy[k] = xb[(int64_t)i * 3 + 1];
        qz[k] = xb[(int64_t)i * 3 + 2];
        best[k] = __builtin_inff();
        bj[k] = m_begin;
    }
    const f2 px0 = {qx[0], qx[1]}, py0 = {qy[0], qy[1]}, pz0 = {qz[0], qz[1]};
    const f2 px1 = {qx[2], qx[3]}, py1 = {qy[2], qy[3]}, pz1 = {qz[2], qz[3]};

    for (int m0 = m_begin; m0 < m_end; m0 += kTile) {
        __syncthreads();                                                    // the previous tile has been read
#pragma unroll
        for (int k = 0; k < kTile / kBlock; ++k) {
            const int j = t + k * kBlock, m = m0 + j;
            const bool in = m < m_end;                                      // padding: +inf, whose distance never wins
            lds[0][j] = in ? yb[(int64_t)m * 3 + 0] : __builtin_inff();
            lds[1][j] = in ? yb[(int64_t)m * 3 + 1] : __builtin_inff();
            lds[2][j] = in ? yb[(int64_t)m * 3 + 2] : __builtin_inff();
        }
        __syncthreads();
        const int n_here = min(kTile, (m_end - m0 + kGroup - 1) / kGroup * kGroup);
#pragma unroll 2
        for (int j = 0; j < n_here; j += kGroup) {
            const float4 tx = *reinterpret_cast<const float4*>(&lds[0][j]);
            const float4 ty = *reinterpret_cast<const float4*>(&lds[1][j]);
            const float4 tz = *reinterpret_cast<const float4*>(&lds[2][j]);
            const f2 a0 = dist2_pk(px0, py0, pz0, tx.x, ty.x, tz.x), c0 = dist2_pk(px1, py1, pz1, tx.x, ty.x, tz.x);
            const f2 a1 = dist2_pk(px0, py0, pz0, tx.y, ty.y, tz.y), c1 = dist2_pk(px1, py1, pz1, tx.y, ty.y, tz.y);
            const f2 a2 = dist2_pk(px0, py0, pz0, tx.z, ty.z, tz.z), c2 = dist2_pk(px1, py1, pz1, tx.z, ty.z, tz.z);
            const f2 a3 = dist2_pk(px0, py0, pz0, tx.w, ty.w, tz.w), c3 = dist2_pk(px1, py1, pz1, tx.w, ty.w, tz.w);
            const float g0 = fminf(fminf(a0.x, a1.x), fminf(a2.x, a3.x));
            const float g1 = fminf(fminf(a0.y, a1.y), fminf(a2.y, a3.y));
            const float g2 = fminf(fminf(c0.x, c1.x), fminf(c2.x, c3.x));
            const float g3 = fminf(fminf(c0.y, c1.y), fminf(c2.y, c3.y));
            const int jj = m0 + j;
            if (g0 < best[0]) { best[0] = g0; bj[0] = jj; }
            if (g1 < best[1]) { best[1] = g1; bj[1] = jj; }
            if (g2 < best[2]) { best[2] = g2; bj[2] = jj; }
            if (g3 < best[3]) { best[3] = g3; bj[3] = jj; }
        }
    }
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        const int i = q0 + k * kBlock;
        if (i >= N) continue;
        int win = bj[k];                                                    // stays the range's first index when nothing is finite
        for (int c = kGroup - 1; c >= 0; --c) {
            const int m = bj[k] + c;
            if (m < m_end) {
                const float d = dist2_1(qx[k], qy[k], qz[k], yb[(int64_t)m * 3 + 0], yb[(int64_t)m * 3 + 1], yb[(int64_t)m * 3 + 2]);
                if (d == best[k]) win = m;                                  // descending c: the lowest equal index is kept
            }
        }
        const int64_t o = (int64_t)b * N + i;
        if (splits == 1) {
            dist2[o] = best[k];
            idx[o] = win;
        } else {
            atomicMin(&keys[o], ((unsigned long long)__float_as_uint(best[k]) << 32) | (unsigned)win);
        }
    }
}

__global__ __launch_bounds__(kBlock) void nn_unpack_kernel(const unsigned long long* __restrict__ keys, int64_t n, int N,
                                                           const int* __restrict__ y_len, const int* __restrict__ active,
                                                           float* __restrict__ dist2, int* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if ((active && !active[i / N]) || (y_len && y_len[i / N] < 1)) return;  // no search ran: dist2 / idx keep their bits
    const unsigned long long k = keys[i];
    dist2[i] = __uint_as_float((unsigned)(k >> 32));
    idx[i] = (int)(unsigned)k;
}

__global__ __launch_bounds__(kBlock) void chamfer_bwd_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                             const int* __restrict__ idx, const float* __restrict__ grad_dist,
                                                             int64_t total, int N, int M, float* __restrict__ grad_x,
                                                             float* __restrict__ grad_y) {
    const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (o >= total) return;
    const int j = idx[o];
    if (j < 0 || j >= M) return;                                            // never read through a bad index
    const int64_t b = o / N;
    const int64_t oy = (b * M + j) * 3;
    const float g = 2.0f * grad_dist[o];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = g * (x[o * 3 + c] - y[oy + c]);
        grad_x[o * 3 + c] += v;
        atomicAdd(&grad_y[oy + c], -v);
    }
}

// partial sums of one workgroup: k < 16 the moments (x0 non-null), k == 16 the squared residual (xt non-null)
__global__ __launch_bounds__(kBlock) void icp_partial_kernel(const float* __restrict__ x0, const float* __restrict__ y,
                                                             const int* __restrict__ idx, const float* __restrict__ xt, int N,
                                                             int M, int nblk, const int* __restrict__ y_len,
                                                             const int* __restrict__ active, double* __restrict__ partials) {
    __shared__ double lds[kBlock / 64][kNSum];
    const int b = blockIdx.x / nblk, k = blockIdx.x - b * nblk;
    if (active && !active[b]) return;                                       // skipped: icp_final_kernel skips it as well
    const int len = y_len ? min(y_len[b], M) : M;                           // ragged: an index into the padding is a bad index
    const int64_t ob = (int64_t)b * N;
    const float* yb = y + (int64_t)b * M * 3;
    double acc[kNSum];
#pragma unroll
    for (int q = 0; q < kNSum; ++q) acc[q] = 0.0;
    for (int i = k * kBlock + threadIdx.x; i < N; i += nblk * kBlock) {
        const int j = idx[ob + i];
        if (j < 0 || j >= len) continue;
        const double ty[3] = {(double)yb[(int64_t)j * 3 + 0], (double)yb[(int64_t)j * 3 + 1], (double)yb[(int64_t)j * 3 + 2]};
        if (x0) {
            const double p[3] = {(double)x0[(ob + i) * 3 + 0], (double)x0[(ob + i) * 3 + 1], (double)x0[(ob + i) * 3 + 2]};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[c] += p[c];
                acc[3 + c] += ty[c];
#pragma unroll
                for (int d = 0; d < 3; ++d) acc[6 + 3 * c + d] += p[c] * ty[d];
                acc[15] += p[c] * p[c];
            }
        }
        if (xt) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double e = (double)xt[(ob + i) * 3 + c] - ty[c];
                acc[16] += e * e;
            }
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kNSum; ++q) {
        const double v = wave_add_down(acc[q]);
        if (lane == 0) lds[w][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < kNSum) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < kBlock / 64; ++q) v += lds[q][threadIdx.x];
        partials[(int64_t)blockIdx.x * kNSum + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(64) void icp_final_kernel(const double* __restrict__ partials, int nblk, int has_x0, int has_xt,
                                                       const int* __restrict__ active, double* __restrict__ out) {
    const int q = threadIdx.x;
    if (q >= kNSum || (q < 16 ? !has_x0 : !has_xt) || (active && !active[blockIdx.x])) return;
    const double* p = partials + (int64_t)blockIdx.x * nblk * kNSum;
    double v = 0.0;
    for (int k = 0; k < nblk; ++k) v += p[(int64_t)k * kNSum + q];          // index order: the same bits on every run
    out[(int64_t)blockIdx.x * kNSum + q] = v;
}

__global__ __launch_bounds__(kBlock) void sim3_apply_kernel(const float* __restrict__ x, const float* __restrict__ rts,
                                                            int64_t total, int N, const int* __restrict__ active,
                                                            float* __restrict__ out) {
    const int64_t o = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (o >= total) return;
    if (active && !active[o / N]) return;                                   // skipped: out keeps its bits
    const float* p = rts + (o / N) * 13;
    const float a = x[o * 3 + 0], b = x[o * 3 + 1], c = x[o * 3 + 2], s = p[12];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float v = __builtin_fmaf(c, p[6 + d], __builtin_fmaf(b, p[3 + d], a * p[d]));
        out[o * 3 + d] = __builtin_fmaf(s, v, p[9 + d]);
    }
}

bool ps_shape_ok(int64_t B, int64_t N, int64_t M) {
    if (B < 1 || M < 1 || N < 0) return false;
    return (double)B * (double)N < 2147483648.0 && (double)B * (double)M < 2147483648.0;
}

void nn_plan(int64_t B, int64_t N, int64_t M, int* nblk, int* splits, int* range) {
    *nblk = (int)((N + kQB - 1) / kQB);
    const int64_t blocks = B * (int64_t)*nblk;
    const int64_t tiles = (M + kTile - 1) / kTile;
    int64_t s = blocks > 0 ? (kTargetBlocks + blocks - 1) / blocks : 1;
    s = s < 1 ? 1 : (s > tiles ? tiles : s);
    const int64_t tiles_per = (tiles + s - 1) / s;
    *range = (int)(tiles_per * kTile);
    *splits = (int)((tiles + tiles_per - 1) / tiles_per);                   // no empty range
}

}   // namespace

extern "C" int32_t moda_nn_splits(int64_t B, int64_t N, int64_t M, int64_t* range) {
    if (!ps_shape_ok(B, N, M) || N == 0) {
        if (range) *range = M;
        return 1;
    }
    int nblk, splits, rg;
    nn_plan(B, N, M, &nblk, &splits, &rg);
    if (range) *range = rg;
    return splits;
}

// the dense entry passes y_len = active = NULL: one launcher, so the ragged route with full lengths runs the same plan and the
// same instructions as the dense one
static int nn_launch(const float* x, const float* y, int64_t B, int64_t N, int64_t M, const int32_t* y_len, const int32_t* active,
                     float* dist2, int32_t* idx, uint64_t* keys, void* stream) {
    if (!ps_shape_ok(B, N, M)) return MODA_ESHAPE;
    if (N == 0) return 0;
    if (!x || !y || !dist2 || !idx) return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int nblk, splits, range;
    nn_plan(B, N, M, &nblk, &splits, &range);
    if (!keys) {                                                            // no workspace: one range
        splits = 1;
        range = (int)((M + kTile - 1) / kTile) * kTile;
    }
    if (splits > 1) {
        hipError_t e = hipMemsetAsync(keys, 0xFF, sizeof(uint64_t) * (size_t)(B * N), st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(nn_kernel, dim3((unsigned)(B * nblk * splits)), dim3(kBlock), 0, st, x, y, (int)N, (int)M, nblk, splits,
                       range, y_len, active, dist2, idx, (unsigned long long*)keys);
    if (splits > 1)
        hipLaunchKernelGGL(nn_unpack_kernel, dim3(nblocks(B * N, kBlock)), dim3(kBlock), 0, st, (const unsigned long long*)keys,
                           B * N, (int)N, y_len, active, dist2, idx);
    return (int)hipGetLastError();
}

extern "C" int moda_nn_fwd(const float* x, const float* y, int64_t B, int64_t N, int64_t M, float* dist2, int32_t* idx,
                           uint64_t* keys, void* stream) {
    return nn_launch(x, y, B, N, M, nullptr, nullptr, dist2, idx, keys, stream);
}

extern "C" int moda_nn_fwd_ragged(const float* x, const float* y, int64_t B, int64_t N, int64_t M_max, const int32_t* y_len,
                                  const int32_t* active, float* dist2, int32_t* idx, uint64_t* keys, void* stream) {
    if (ps_shape_ok(B, N, M_max) && N > 0 && !y_len) return MODA_EINVAL;
    return nn_launch(x, y, B, N, M_max, y_len, active, dist2, idx, keys, stream);
}

extern "C" int moda_chamfer_bwd(const float* x, const float* y, const int32_t* idx, const float* grad_dist, int64_t B, int64_t N,
                                int64_t M, float* grad_x, float* grad_y, void* stream) {
    if (!ps_shape_ok(B, N, M)) return MODA_ESHAPE;
    if (N == 0) return 0;
    if (!x || !y || !idx || !grad_dist || !grad_x || !grad_y) return MODA_EINVAL;
    hipLaunchKernelGGL(chamfer_bwd_kernel, dim3(nblocks(B * N, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, x, y, idx, grad_dist,
                       B * N, (int)N, (int)M, grad_x, grad_y);
    return (int)hipGetLastError();
}

static int icp_moments_launch(const float* x0, const float* y, const int32_t* idx, const float* xt, int64_t B, int64_t N, int64_t M,
                              const int32_t* y_len, const int32_t* active, double* partials, double* sums, void* stream) {
    if (!ps_shape_ok(B, N, M) || N < 1) return MODA_ESHAPE;
    const int nblk = (int)((N + kQB - 1) / kQB) < kIcpMaxBlocks ? (int)((N + kQB - 1) / kQB) : kIcpMaxBlocks;
    if ((double)B * nblk >= 2147483648.0) return MODA_ESHAPE;
    if (!y || !idx || (!x0 && !xt) || !partials || !sums) return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(icp_partial_kernel, dim3((unsigned)(B * nblk)), dim3(kBlock), 0, st, x0, y, idx, xt, (int)N, (int)M, nblk,
                       y_len, active, partials);
    hipLaunchKernelGGL(icp_final_kernel, dim3((unsigned)B), dim3(64), 0, st, (const double*)partials, nblk, x0 ? 1 : 0, xt ? 1 : 0,
                       active, sums);
    return (int)hipGetLastError();
}

extern "C" int moda_icp_moments(const float* x0, const float* y, const int32_t* idx, const float* xt, int64_t B, int64_t N,
                                int64_t M, double* partials, double* sums, void* stream) {
    return icp_moments_launch(x0, y, idx, xt, B, N, M, nullptr, nullptr, partials, sums, stream);
}

extern "C" int moda_icp_moments_ragged(const float* x0, const float* y, const int32_t* idx, const float* xt, int64_t B, int64_t N,
                                       int64_t M_max, const int32_t* y_len, const int32_t* active, double* partials, double* sums,
                                       void* stream) {
    if (ps_shape_ok(B, N, M_max) && N >= 1 && !y_len) return MODA_EINVAL;
    return icp_moments_launch(x0, y, idx, xt, B, N, M_max, y_len, active, partials, sums, stream);
}

static int sim3_launch(const float* x, const float* rts, int64_t B, int64_t N, const int32_t* active, float* out, void* stream) {
    if (B < 1 || N < 0 || (double)B * (double)N >= 2147483648.0) return MODA_ESHAPE;
    if (N == 0) return 0;
    if (!x || !rts || !out) return MODA_EINVAL;
    hipLaunchKernelGGL(sim3_apply_kernel, dim3(nblocks(B * N, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, x, rts, B * N, (int)N,
                       active, out);
    return (int)hipGetLastError();
}

extern "C" int moda_sim3_apply(const float* x, const float* rts, int64_t B, int64_t N, float* out, void* stream) {
    return sim3_launch(x, rts, B, N, nullptr, out, stream);
}

extern "C" int moda_sim3_apply_masked(const float* x, const float* rts, int64_t B, int64_t N, const int32_t* active, float* out,
                                      void* stream) {
    return sim3_launch(x, rts, B, N, active, out, stream);
}
