// Camera kernels (include/moda_hip_cams.h): what follows extract_cams in the reference's recipe, without a host read.
//
//   fill      save_cams' per-frame block: one workgroup a video walks its frames in chunks of 256, left to right for the last
//             valid frame at or before each frame, right to left for the first at or after it.  Inside a wave both are a ballot
//             and a count of leading / trailing zeros; across waves and chunks a carried index.  Then the closer of the two (the
//             lower on a tie) lends its rotation, the translation is scaled, and the frame-table rows are written.
//   sim3      align_sim3 in one workgroup: float64 sums over the frames in a fixed tree, a 4 x 4 cyclic Jacobi in one lane for
//             scipy's Rotation.mean, the aligned cameras, the rotation errors and their statistics; the median by rank count
//             (block_median), which the glyph scale of draw_cams reuses.
//   hull      visual_hull_align: one lane per lattice point, k fastest, the views' camera rows staged in LDS a tile at a time;
//             selection count and float64 coordinate sums through a two-stage tree; a second launch forms the centre.
//   glyphs    draw_cams / draw_cams_pair as instancing launches.
// Device memory is written by plain vector stores only; no atomics, no device-side assert or print.  Contraction is off for
// the whole file: the float64 restatements (tests/cams_numpy.py) round every product and sum on their own.
#include "lanes.h"
#include "moda_hip_cams.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = MODA_CAM_BLOCK;
constexpr int kWaves = kBlock / 64;
constexpr int kViewTile = MODA_CAM_VIEW_TILE;
constexpr int kPart = MODA_CAM_PART_FIELDS;

// the sum of a workgroup's values, in every lane: the xor butterfly of each wave, then the waves in index order
template <class T>
DEVINL T block_sum(T v, T* lds) {
    v = wave_add(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T t = lds[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) t += lds[w];
    __syncthreads();
    return t;
}

// np.median of the eligible elements of x[0, n) by rank count, one workgroup: rank(i) = #{j eligible: x[j] < x[i], or x[j] == x[i]
// and j < i}; the elements of rank (m - 1) / 2 and m / 2 are written by their owners (each rank has one owner) into s_pair, their
// float64 mean is returned in every lane (NaN when nothing is eligible).  positive_only: eligible = x > 0.  x must be visible to
// the workgroup (a __syncthreads() after its stores).
DEVINL double block_median(const float* x, int n, bool positive_only, float* s_pair, int* s_m) {
    if (threadIdx.x == 0) {
        *s_m = 0;
        s_pair[0] = s_pair[1] = __int_as_float(0x7fc00000);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kBlock) {
        const float vi = x[i];
        if (positive_only && !(vi > 0.f)) continue;
        int m = 0, rank = 0;
        for (int j = 0; j < n; ++j) {
            const float vj = x[j];
            const bool e = !positive_only || vj > 0.f;
            m += e;
            rank += e && (vj < vi || (vj == vi && j < i));
        }
        *s_m = m;                                                 // the same value from every owner
        if (rank == (m - 1) / 2) s_pair[0] = vi;
        if (rank == m / 2) s_pair[1] = vi;
    }
    __syncthreads();
    const double med = *s_m > 0 ? 0.5 * ((double)s_pair[0] + (double)s_pair[1]) : (double)__int_as_float(0x7fc00000);
    __syncthreads();
    return med;
}

// ---- fill ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cam_fill_kernel(const float* __restrict__ rtk, const uint8_t* __restrict__ valid,
                                                          const int* __restrict__ off, long long N, int fill, float scale,
                                                          float* __restrict__ out, int* __restrict__ src, int* __restrict__ n_valid,
                                                          int* __restrict__ rows, float* __restrict__ tab_rtk,
                                                          float* __restrict__ tab_raw, long long M) {
    __shared__ int s_edge[kWaves], s_pop[kWaves];
    const int v = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long lo = off[v], hi = off[v + 1];
    if (lo < 0 || hi > N || hi < lo) return;                                       // workgroup-uniform
    const int len = (int)(hi - lo), chunks = (len + kBlock - 1) / kBlock;
    // left to right: the last valid frame at or before each frame (an index inside the video, -1: none), parked in src
    int carry = -1, cnt = 0;
    for (int c = 0; c < chunks; ++c) {
        const int base = c * kBlock + wave * 64, r = base + lane;
        const unsigned long long m = __ballot(r < len && valid[lo + r] != 0);
        if (lane == 0) {
            s_edge[wave] = m ? base + 63 - __clzll((long long)m) : -1;
            s_pop[wave] = __popcll(m);
        }
        __syncthreads();
        const unsigned long long mine = m & ((2ull << lane) - 1ull);
        int left = mine ? base + 63 - __clzll((long long)mine) : -1;
        for (int w = wave - 1; left < 0 && w >= 0; --w) left = s_edge[w];
        if (left < 0) left = carry;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (s_edge[w] >= 0) carry = s_edge[w];
            cnt += s_pop[w];
        }
        if (r < len) src[lo + r] = left;
        __syncthreads();
    }
    if (threadIdx.x == 0) n_valid[v] = cnt;
    // right to left: the first valid frame at or after each frame, then the closer of the two
    carry = -1;
    for (int c = chunks - 1; c >= 0; --c) {
        const int base = c * kBlock + wave * 64, r = base + lane;
        const bool ok = r < len && valid[lo + r] != 0;
        const unsigned long long m = __ballot(ok);
        if (lane == 0) s_edge[wave] = m ? base + __ffsll((long long)m) - 1 : -1;
        __syncthreads();
        const unsigned long long mine = m & (~0ull << lane);
        int right = mine ? base + __ffsll((long long)mine) - 1 : -1;
        for (int w = wave + 1; right < 0 && w < kWaves; ++w) right = s_edge[w];
        if (right < 0) right = carry;
#pragma unroll
        for (int w = kWaves - 1; w >= 0; --w)
            if (s_edge[w] >= 0) carry = s_edge[w];
        if (r < len) {
            const long long i = lo + r;
            const int left = src[i];                                                // this lane's own store
            int pick = r;
            if (fill && !ok) {
                if (left >= 0 && right >= 0) pick = (r - left <= right - r) ? left : right;
                else if (left >= 0) pick = left;
                else if (right >= 0) pick = right;
            }
            src[i] = (int)(lo + pick);
            const float* own = rtk + i * 16;
            const float* rot = rtk + (lo + pick) * 16;
            float row[16];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) row[a * 4 + b] = rot[a * 4 + b];
                row[a * 4 + 3] = own[a * 4 + 3] * scale;
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) row[12 + b] = own[12 + b];
#pragma unroll
            for (int e = 0; e < 16; ++e) out[i * 16 + e] = row[e];
            const long long trow = i + v;
            if (rows) rows[i] = (int)trow;
            if (tab_rtk) {
                for (int dup = 0; dup < (r == len - 1 ? 2 : 1); ++dup) {
                    const long long t = trow + dup;
                    if (t >= M) break;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
#pragma unroll
                        for (int b = 0; b < 4; ++b) tab_raw[t * 12 + a * 4 + b] = row[a * 4 + b];
#pragma unroll
                        for (int b = 0; b < 3; ++b) tab_rtk[t * 16 + a * 4 + b] = row[a * 4 + b];
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---- sim3 ---------------------------------------------------------------------------------------------------------------------
// A <- J^T A J for the (p, q) plane of a symmetric 4 x 4 matrix, V <- V J (cyclic Jacobi; Golub & Van Loan, Matrix Computations,
// section 8.5: the smaller root t of t^2 + 2 theta t - 1 = 0 zeroes A[p][q])
template <int P, int Q>
DEVINL void jacobi_pair(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

// scipy's Rotation.from_matrix for one matrix M (row major) -> (x, y, z, w), normalised
DEVINL void mat_to_quat(const double (&M)[3][3], double (&q)[4]) {
    const double tr = M[0][0] + M[1][1] + M[2][2];
    const double dec[4] = {M[0][0], M[1][1], M[2][2], tr};
    int ch = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (dec[k] > dec[ch]) ch = k;
    if (ch == 3) {
        q[0] = M[2][1] - M[1][2];
        q[1] = M[0][2] - M[2][0];
        q[2] = M[1][0] - M[0][1];
        q[3] = 1.0 + tr;
    } else {
        const int i = ch, j = (i + 1) % 3, k = (j + 1) % 3;
        double e[3];
        e[i] = 1.0 - tr + 2.0 * M[i][i];
        e[j] = M[j][i] + M[i][j];
        e[k] = M[k][i] + M[i][k];
        q[0] = e[0];
        q[1] = e[1];
        q[2] = e[2];
        q[3] = M[k][j] - M[j][k];
    }
    const double nrm = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = q[c] / nrm;
}

DEVINL void load_rt(const float* p, double (&R)[3][3], double (&t)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) R[a][b] = (double)p[a * 4 + b];
        t[a] = (double)p[a * 4 + 3];
    }
}

DEVINL double norm3(const double (&t)[3]) { return sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]); }

__global__ __launch_bounds__(kBlock) void cam_sim3_kernel(const float* __restrict__ ra, const float* __restrict__ rb,
                                                          const uint8_t* __restrict__ inl, const float* __restrict__ err, int n,
                                                          float* __restrict__ bout, double* __restrict__ fit, float* __restrict__ so3,
                                                          double* __restrict__ stats, uint8_t* __restrict__ used,
                                                          int* __restrict__ status) {
    __shared__ double s_d[kWaves];
    __shared__ int s_i[kWaves];
    __shared__ float s_f[kWaves];
    __shared__ double s_fit[10];
    __shared__ float s_pair[2];
    __shared__ int s_m;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // who is used: the inliers; without one, the frame of smallest err_valid
    int fallback = -1;
    if (inl) {
        int c = 0;
        for (int i = tid; i < n; i += kBlock) c += inl[i] != 0;
        if (block_sum(c, s_i) == 0) {
            float best = __builtin_huge_valf();
            int at = 0x7fffffff;
            bool any = false;
            for (int i = tid; i < n; i += kBlock) {
                const float e = err[i];
                if (e < best || (!any && e == best)) { best = e; at = i; any = true; }
            }
            const float all = wave_all(best, [](float a, float b) { return b < a ? b : a; });
            if (lane == 0) s_f[wave] = all;
            __syncthreads();
            float g = s_f[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) g = s_f[w] < g ? s_f[w] : g;
            int cand = (any && best == g) ? at : 0x7fffffff;
            cand = wave_all(cand, [](int a, int b) { return b < a ? b : a; });
            if (lane == 0) s_i[wave] = cand;
            __syncthreads();
            fallback = s_i[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) fallback = s_i[w] < fallback ? s_i[w] : fallback;
            if (fallback == 0x7fffffff) fallback = 0;                              // every err_valid is NaN
            __syncthreads();
        }
    }
    // sums over the used frames: the 10 entries of q q^T, dscale, the count; zero-norm translations over all frames
    double acc[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) acc[k] = 0.0;
    int n_used = 0, n_zero = 0;
    for (int i = tid; i < n; i += kBlock) {
        double Ra[3][3], Rb[3][3], ta[3], tb[3], D[3][3], q[4];
        load_rt(ra + (long long)i * 16, Ra, ta);
        load_rt(rb + (long long)i * 16, Rb, tb);
        const double nb = norm3(tb);
        n_zero += nb == 0.0;
        const bool u = inl ? (fallback >= 0 ? i == fallback : inl[i] != 0) : true;
        used[i] = u ? 1 : 0;
        if (!u) continue;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) D[a][b] = (Rb[0][a] * Ra[0][b] + Rb[1][a] * Ra[1][b]) + Rb[2][a] * Ra[2][b];
        mat_to_quat(D, q);
        int k = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a; b < 4; ++b) acc[k++] += q[a] * q[b];
        acc[10] += norm3(ta) / nb;
        ++n_used;
    }
#pragma unroll
    for (int k = 0; k < 11; ++k) acc[k] = block_sum(acc[k], s_d);
    n_used = block_sum(n_used, s_i);
    n_zero = block_sum(n_zero, s_i);
    if (tid == 0) {
        double A[4][4], V[4][4];
        int k = 0;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = a; b < 4; ++b) {
                A[a][b] = A[b][a] = acc[k++];
                V[a][b] = V[b][a] = a == b ? 1.0 : 0.0;
            }
        int sweeps = 0;
        for (; sweeps < MODA_CAM_JACOBI_SWEEPS; ++sweeps) {
            const double offd = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[0][3]) + fabs(A[1][2]) + fabs(A[1][3]) + fabs(A[2][3]);
            if (offd == 0.0) break;
            jacobi_pair<0, 1>(A, V);
            jacobi_pair<0, 2>(A, V);
            jacobi_pair<0, 3>(A, V);
            jacobi_pair<1, 2>(A, V);
            jacobi_pair<1, 3>(A, V);
            jacobi_pair<2, 3>(A, V);
        }
        int top = 0;
#pragma unroll
        for (int c = 1; c < 4; ++c)
            if (A[c][c] > A[top][top]) top = c;
        double second = -__builtin_huge_val();
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c != top && A[c][c] > second) second = A[c][c];
        double x = V[0][0], y = V[1][0], z = V[2][0], w = V[3][0];
#pragma unroll
        for (int c = 1; c < 4; ++c)
            if (c == top) { x = V[0][c]; y = V[1][c]; z = V[2][c]; w = V[3][c]; }
        const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w, xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
        s_fit[0] = ((x2 - y2) - z2) + w2;
        s_fit[1] = 2.0 * (xy - zw);
        s_fit[2] = 2.0 * (xz + yw);
        s_fit[3] = 2.0 * (xy + zw);
        s_fit[4] = ((-x2 + y2) - z2) + w2;
        s_fit[5] = 2.0 * (yz - xw);
        s_fit[6] = 2.0 * (xz - yw);
        s_fit[7] = 2.0 * (yz + xw);
        s_fit[8] = ((-x2 - y2) + z2) + w2;
        s_fit[9] = acc[10] / (double)n_used;
#pragma unroll
        for (int c = 0; c < 10; ++c) fit[c] = s_fit[c];
        fit[10] = A[top][top];
        fit[11] = second;
        status[MODA_CAM_SIM3_ZERO_NORM] = n_zero;
        status[MODA_CAM_SIM3_FALLBACK] = fallback >= 0 ? 1 : 0;
        status[MODA_CAM_SIM3_USED] = n_used;
        status[MODA_CAM_SIM3_SWEEPS] = sweeps;
    }
    __syncthreads();
    // the aligned cameras and their rotation errors
    const double sc = s_fit[9], lim = 1.0 - 1e-4;
    double esum = 0.0;
    float emax = -__builtin_huge_valf();
    for (int i = tid; i < n; i += kBlock) {
        double Ra[3][3], Rb[3][3], ta[3], tb[3], Rn[3][3];
        load_rt(ra + (long long)i * 16, Ra, ta);
        load_rt(rb + (long long)i * 16, Rb, tb);
        float* o = bout + (long long)i * 16;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                Rn[a][b] = (Rb[a][0] * s_fit[b] + Rb[a][1] * s_fit[3 + b]) + Rb[a][2] * s_fit[6 + b];
                o[a * 4 + b] = (float)Rn[a][b];
            }
            o[a * 4 + 3] = (float)(tb[a] * sc);
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) o[12 + b] = rb[(long long)i * 16 + 12 + b];
        double tr = 0.0;                                                            // trace(Ra Rn^T) = sum_ab Ra[a][b] Rn[a][b]
#pragma unroll
        for (int a = 0; a < 3; ++a) tr += (Ra[a][0] * Rn[a][0] + Ra[a][1] * Rn[a][1]) + Ra[a][2] * Rn[a][2];
        double cs = (tr - 1.0) / 2.0;
        cs = cs < -lim ? -lim : (cs > lim ? lim : cs);
        const float e = (float)(acos(cs) / 3.141592653589793 * 180.0);
        so3[i] = e;
        esum += (double)e;
        emax = e > emax ? e : emax;                                                  // a NaN error is not a maximum
    }
    esum = block_sum(esum, s_d);
    emax = wave_all(emax, [](float a, float b) { return b > a ? b : a; });
    if (lane == 0) s_f[wave] = emax;
    __syncthreads();
    emax = s_f[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) emax = s_f[w] > emax ? s_f[w] : emax;
    const double mean = esum / (double)n;
    double ss = 0.0;
    for (int i = tid; i < n; i += kBlock) {
        const double d = (double)so3[i] - mean;                                      // this lane's own stores
        ss += d * d;
    }
    ss = block_sum(ss, s_d);                                                          // (its barriers make so3 visible to all)
    const double med = block_median(so3, n, false, s_pair, &s_m);
    if (tid == 0) {
        stats[0] = (double)emax;
        stats[1] = med;
        stats[2] = mean;
        stats[3] = sqrt(ss / (double)(n - 1));                                       // n = 1: 0 / 0 = NaN, as torch's std
    }
}

// ---- hull ---------------------------------------------------------------------------------------------------------------------
// a view's row in LDS: R (9), t (3), fx, fy, px, py of the composed intrinsics
struct HullCam { float R[9], t[3], k[4]; };

// the camera centre entry c[a] = -(R^T t)[a] in fp32, the reference's order
DEVINL float cam_centre(const float* p, int a) { return -((p[a] * p[3] + p[4 + a] * p[7]) + p[8 + a] * p[11]); }

// bound = mean |c| over all 3 V entries, the same bits in every workgroup
DEVINL float hull_bound(const float* rtk, int V, double* lds) {
    double s = 0.0;
    for (int v = threadIdx.x; v < V; v += kBlock) {
        const float* p = rtk + (long long)v * 16;
        s += ((double)fabsf(cam_centre(p, 0)) + (double)fabsf(cam_centre(p, 1))) + (double)fabsf(cam_centre(p, 2));
    }
    return (float)(block_sum(s, lds) / (double)(3 * (long long)V));
}

DEVINL float lattice(int i, int G, float bound) {
    if (i == G - 1) return bound;
    const double b = (double)bound, step = (b - (-b)) / (double)(G - 1);
    return (float)((double)i * step + (-b));
}

DEVINL double mask_at(const float* m, long long i) { return (double)m[i]; }
DEVINL double mask_at(const uint8_t* m, long long i) { return (double)m[i]; }

template <class MaskT>
__global__ __launch_bounds__(kBlock) void cam_hull_vote_kernel(const float* __restrict__ rtk, const float* __restrict__ kaug,
                                                               const MaskT* __restrict__ masks, int V, int h, int w, int G,
                                                               float* __restrict__ scores, double* __restrict__ part) {
    __shared__ HullCam s_cam[kViewTile];
    __shared__ double s_d[kWaves];
    const int tid = threadIdx.x;
    const float bound = hull_bound(rtk, V, s_d);
    const long long P = (long long)G * G * G, p = (long long)blockIdx.x * kBlock + tid;
    const bool live = p < P;
    const long long pc = live ? p : P - 1;
    const int pi = (int)(pc / ((long long)G * G)), pj = (int)((pc / G) % G), pk = (int)(pc % G);
    const double X = (double)lattice(pi, G, bound), Y = (double)lattice(pj, G, bound), Z = (double)lattice(pk, G, bound);
    const double dw = (double)w, dh = (double)h;
    double score = 0.0, bad = 0.0;
    for (int v0 = 0; v0 < V; v0 += kViewTile) {
        const int nv = min(kViewTile, V - v0);
        __syncthreads();
        if (tid < nv) {                                                             // fp32, the reference's order
            const float* r = rtk + (long long)(v0 + tid) * 16;
            const float* ka = kaug + (long long)(v0 + tid) * 4;
            HullCam c;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = 0; b < 3; ++b) c.R[a * 3 + b] = r[a * 4 + b];
                c.t[a] = r[a * 4 + 3];
            }
            const float ix = 1.f / ka[0], iy = 1.f / ka[1], ox = -ka[2] / ka[0], oy = -ka[3] / ka[1];
            c.k[0] = ix * r[12];
            c.k[1] = iy * r[13];
            c.k[2] = ix * r[14] + ox;
            c.k[3] = iy * r[15] + oy;
            s_cam[tid] = c;
        }
        __syncthreads();
        for (int v = 0; v < nv; ++v) {
            const HullCam& c = s_cam[v];
            const double xc = (((double)c.R[0] * X + (double)c.R[1] * Y) + (double)c.R[2] * Z) + (double)c.t[0];
            const double yc = (((double)c.R[3] * X + (double)c.R[4] * Y) + (double)c.R[5] * Z) + (double)c.t[1];
            const double zc = (((double)c.R[6] * X + (double)c.R[7] * Y) + (double)c.R[8] * Z) + (double)c.t[2];
            const double den = 1e-6 + zc;
            const double px = ((double)c.k[0] * xc + (double)c.k[2] * zc) / den, py = ((double)c.k[1] * yc + (double)c.k[3] * zc) / den;
            const double gx = px / dw * 2.0 - 1.0, gy = py / dh * 2.0 - 1.0;
            const double fx = ((gx + 1.0) * dw - 1.0) / 2.0, fy = ((gy + 1.0) * dh - 1.0) / 2.0;
            if (!(fabs(fx) < __builtin_huge_val()) || !(fabs(fy) < __builtin_huge_val())) {     // inf or NaN
                bad += 1.0;
                continue;
            }
            const double x0 = floor(fx), y0 = floor(fy);
            if (x0 < -1.0 || x0 > dw - 1.0 || y0 < -1.0 || y0 > dh - 1.0) continue;               // all four corners outside
            const int xi = (int)x0, yi = (int)y0;
            const double ax = fx - x0, ay = fy - y0, bx = (x0 + 1.0) - fx, by = (y0 + 1.0) - fy;
            const long long base = (long long)(v0 + v) * h * w;
            const bool inx0 = xi >= 0, inx1 = xi + 1 < w, iny0 = yi >= 0, iny1 = yi + 1 < h;
            double s = 0.0;
            if (inx0 && iny0) s += mask_at(masks, base + (long long)yi * w + xi) * (bx * by);
            if (inx1 && iny0) s += mask_at(masks, base + (long long)yi * w + xi + 1) * (ax * by);
            if (inx0 && iny1) s += mask_at(masks, base + (long long)(yi + 1) * w + xi) * (bx * ay);
            if (inx1 && iny1) s += mask_at(masks, base + (long long)(yi + 1) * w + xi + 1) * (ax * ay);
            score += s;
        }
    }
    const bool sel = live && score > 0.8 * (double)V;
    if (live && scores) scores[p] = (float)score;
    const double cnt = block_sum(sel ? 1.0 : 0.0, s_d), sx = block_sum(sel ? X : 0.0, s_d), sy = block_sum(sel ? Y : 0.0, s_d),
                 sz = block_sum(sel ? Z : 0.0, s_d), nb = block_sum(live ? bad : 0.0, s_d);
    if (tid == 0) {
        double* o = part + (long long)blockIdx.x * kPart;
        o[0] = cnt;
        o[1] = sx;
        o[2] = sy;
        o[3] = sz;
        o[4] = nb;
    }
}

__global__ __launch_bounds__(kBlock) void cam_hull_apply_kernel(const float* __restrict__ rtk, int V, long long nparts,
                                                                const double* __restrict__ part, float* __restrict__ out,
                                                                int* __restrict__ status) {
    __shared__ double s_d[kWaves];
    double acc[kPart];
#pragma unroll
    for (int k = 0; k < kPart; ++k) acc[k] = 0.0;
    for (long long b = threadIdx.x; b < nparts; b += kBlock)
#pragma unroll
        for (int k = 0; k < kPart; ++k) acc[k] += part[b * kPart + k];
#pragma unroll
    for (int k = 0; k < kPart; ++k) acc[k] = block_sum(acc[k], s_d);
    const bool empty = !(acc[0] > 0.0);
    const double ctr[3] = {empty ? 0.0 : acc[1] / acc[0], empty ? 0.0 : acc[2] / acc[0], empty ? 0.0 : acc[3] / acc[0]};
    if (threadIdx.x == 0) {
        status[MODA_CAM_HULL_NONFINITE] = acc[4] > 2147483647.0 ? 2147483647 : (int)acc[4];
        status[MODA_CAM_HULL_EMPTY] = empty ? 1 : 0;
        status[MODA_CAM_HULL_SELECTED] = (int)acc[0];
        status[3] = 0;
    }
    for (int v = threadIdx.x; v < V; v += kBlock) {
        const float* p = rtk + (long long)v * 16;
        float* o = out + (long long)v * 16;
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e] = p[e];
        if (empty) continue;
        const double d[3] = {(double)cam_centre(p, 0) - ctr[0], (double)cam_centre(p, 1) - ctr[1], (double)cam_centre(p, 2) - ctr[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a)
            o[a * 4 + 3] = (float)(-(((double)p[a * 4] * d[0] + (double)p[a * 4 + 1] * d[1]) + (double)p[a * 4 + 2] * d[2]));
    }
}

// ---- glyphs -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void cam_tnorm_median_kernel(const float* __restrict__ rtk, int n, float* __restrict__ work,
                                                                  float* __restrict__ out) {
    __shared__ float s_pair[2];
    __shared__ int s_m;
    for (int i = threadIdx.x; i < n; i += kBlock) {
        const float* p = rtk + (long long)i * 16;
        const double t[3] = {(double)p[3], (double)p[7], (double)p[11]};
        work[i] = (float)norm3(t);
    }
    __syncthreads();
    const double med = block_median(work, n, true, s_pair, &s_m);
    if (threadIdx.x == 0) out[0] = (float)med;
}

__global__ __launch_bounds__(kBlock) void cam_glyphs_kernel(const float* __restrict__ rtk, long long total, int Nv,
                                                            const float* __restrict__ tmpl, const float* __restrict__ scale,
                                                            float factor, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    const long long i = e / Nv;
    const int t = (int)(e - i * Nv);
    const float* p = rtk + i * 16;
    const double radius = (double)(factor * scale[0]);
    const double g[3] = {radius * (double)tmpl[t * 3] - (double)p[3], radius * (double)tmpl[t * 3 + 1] - (double)p[7],
                         radius * (double)tmpl[t * 3 + 2] - (double)p[11]};
#pragma unroll
    for (int a = 0; a < 3; ++a)                                                      // R^T (radius v - t)
        out[e * 3 + a] = (float)(((double)p[a] * g[0] + (double)p[4 + a] * g[1]) + (double)p[8 + a] * g[2]);
}

__global__ __launch_bounds__(kBlock) void cam_links_kernel(const float* __restrict__ c1, const float* __restrict__ c2, int n, float half,
                                                           float* __restrict__ out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float* p = c1 + (long long)i * 16;
    const float* q = c2 + (long long)i * 16;
    double e0[3], e1[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e0[a] = -(((double)p[a] * (double)p[3] + (double)p[4 + a] * (double)p[7]) + (double)p[8 + a] * (double)p[11]);
        e1[a] = -(((double)q[a] * (double)q[3] + (double)q[4 + a] * (double)q[7]) + (double)q[8 + a] * (double)q[11]);
        d[a] = e1[a] - e0[a];
    }
    double u[3] = {1.0, 0.0, 0.0}, w[3] = {0.0, 1.0, 0.0};
    const double len = norm3(d);
    if (len > 0.0) {
        const int k = fabs(d[0]) <= fabs(d[1]) ? (fabs(d[0]) <= fabs(d[2]) ? 0 : 2) : (fabs(d[1]) <= fabs(d[2]) ? 1 : 2);
        const double ax[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        double c[3] = {d[1] * ax[2] - d[2] * ax[1], d[2] * ax[0] - d[0] * ax[2], d[0] * ax[1] - d[1] * ax[0]};
        const double nc = norm3(c);
#pragma unroll
        for (int a = 0; a < 3; ++a) u[a] = c[a] / nc;
        double f[3] = {d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0]};
        const double nf = norm3(f);
#pragma unroll
        for (int a = 0; a < 3; ++a) w[a] = f[a] / nf;
    }
    const double hf = (double)half;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const double su = (c & 2) ? hf : -hf, sw = (c & 1) ? hf : -hf;
#pragma unroll
        for (int a = 0; a < 3; ++a) out[((long long)i * 8 + c) * 3 + a] = (float)(((c & 4) ? e1[a] : e0[a]) + su * u[a] + sw * w[a]);
    }
}

}   // namespace

extern "C" int moda_cam_fill(const float* rtk, const uint8_t* valid, const int32_t* frame_offset, int64_t n_videos, int64_t N,
                             int32_t fill, float scale, float* rtk_out, int32_t* src, int32_t* n_valid, int32_t* rows, float* tab_rtk,
                             float* tab_rt_raw, int64_t M, void* stream) {
    if (N < 1 || n_videos < 1 || N + n_videos >= 0x7fffffffLL) return MODA_ESHAPE;
    if (!rtk || !valid || !frame_offset || !rtk_out || !src || !n_valid || ((tab_rtk != nullptr) != (tab_rt_raw != nullptr)))
        return MODA_EINVAL;
    if (tab_rtk && M < 1) return MODA_ESHAPE;
    hipLaunchKernelGGL(cam_fill_kernel, dim3((unsigned)n_videos), dim3(kBlock), 0, (hipStream_t)stream, rtk, valid, frame_offset,
                       (long long)N, (int)fill, scale, rtk_out, src, n_valid, rows, tab_rtk, tab_rt_raw, (long long)M);
    return (int)hipGetLastError();
}

extern "C" int moda_cam_sim3(const float* roots_a, const float* roots_b, const uint8_t* is_inlier, const float* err_valid, int64_t n,
                             float* b_out, double* fit, float* so3_err, double* stats, uint8_t* inlier_used, int32_t* status,
                             void* stream) {
    if (n < 1 || n > (1 << 24)) return MODA_ESHAPE;
    if (!roots_a || !roots_b || !b_out || !fit || !so3_err || !stats || !inlier_used || !status || (is_inlier && !err_valid))
        return MODA_EINVAL;
    hipLaunchKernelGGL(cam_sim3_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, roots_a, roots_b, is_inlier, err_valid, (int)n,
                       b_out, fit, so3_err, stats, inlier_used, status);
    return (int)hipGetLastError();
}

static bool hull_shape_ok(int64_t V, int64_t G) { return V >= 1 && V <= (1 << 20) && G >= 2 && G <= MODA_CAM_MAX_GRID; }

extern "C" int moda_cam_hull_vote(const float* rtk, const float* kaug, const void* masks, int32_t mask_u8, int64_t V, int64_t h,
                                  int64_t w, int64_t G, float* scores, double* part, void* stream) {
    if (!hull_shape_ok(V, G) || h < 1 || w < 1 || h > 0x7ffffffeLL || w > 0x7ffffffeLL || h * w > (1LL << 40) / V) return MODA_ESHAPE;
    if (!rtk || !kaug || !masks || !part) return MODA_EINVAL;
    const unsigned grid = nblocks(G * G * G, kBlock);
    if (mask_u8)
        hipLaunchKernelGGL(cam_hull_vote_kernel<uint8_t>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, rtk, kaug,
                           (const uint8_t*)masks, (int)V, (int)h, (int)w, (int)G, scores, part);
    else
        hipLaunchKernelGGL(cam_hull_vote_kernel<float>, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, rtk, kaug,
                           (const float*)masks, (int)V, (int)h, (int)w, (int)G, scores, part);
    return (int)hipGetLastError();
}

extern "C" int moda_cam_hull_apply(const float* rtk, int64_t V, int64_t G, const double* part, float* rtk_out, int32_t* status,
                                   void* stream) {
    if (!hull_shape_ok(V, G)) return MODA_ESHAPE;
    if (!rtk || !part || !rtk_out || !status) return MODA_EINVAL;
    hipLaunchKernelGGL(cam_hull_apply_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, rtk, (int)V,
                       (long long)nblocks(G * G * G, kBlock), part, rtk_out, status);
    return (int)hipGetLastError();
}

extern "C" int moda_cam_tnorm_median(const float* rtk, int64_t n, float* work, float* out, void* stream) {
    if (n < 1 || n > (1 << 24)) return MODA_ESHAPE;
    if (!rtk || !work || !out) return MODA_EINVAL;
    hipLaunchKernelGGL(cam_tnorm_median_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, rtk, (int)n, work, out);
    return (int)hipGetLastError();
}

extern "C" int moda_cam_glyphs(const float* rtk, int64_t n, const float* tmpl, int32_t Nv, const float* scale, float factor,
                               float* out, void* stream) {
    if (n < 1 || Nv < 1 || n > 0x7fffffffLL || n * Nv >= 0x7fffffffLL / 3) return MODA_ESHAPE;
    if (!rtk || !tmpl || !scale || !out) return MODA_EINVAL;
    const long long total = n * Nv;
    hipLaunchKernelGGL(cam_glyphs_kernel, dim3(nblocks(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, rtk, total, (int)Nv, tmpl,
                       scale, factor, out);
    return (int)hipGetLastError();
}

extern "C" int moda_cam_links(const float* cam1, const float* cam2, int64_t n, float half, float* out, void* stream) {
    if (n < 1 || n > (1 << 24)) return MODA_ESHAPE;
    if (!cam1 || !cam2 || !out) return MODA_EINVAL;
    hipLaunchKernelGGL(cam_links_kernel, dim3(nblocks(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, cam1, cam2, (int)n, half, out);
    return (int)hipGetLastError();
}
