// The debiased Sinkhorn divergence of geomloss 0.2.4 (SamplesLoss("sinkhorn", p=2, blur, scaling, debias=True), the tensorized
// route of sinkhorn_divergence.py) between two small point clouds, device-resident: the reference's bone-location term
// (nnutils/moda.py:693-695).  Restated from geomloss' published code; geomloss itself is not part of the reference tree, so this
// restatement is unpinned (include/moda_hip.h).
//
//   prep    one workgroup: the joint bounding box, d = |max - min| (max_diameter), the epsilon schedule (epsilon_schedule:
//           [d^2] + [exp(e) for e in arange(2 ln d, 2 ln blur, 2 ln scaling)] + [blur^2]) in double, its length n and the status
//           flags into the workspace header.  The host never sees d: the launch count below does not depend on it.
//   rows    one wavefront per point r of the joined cloud [x; y]: the two softmins of that point -- over the x columns and over
//           the y columns -- by a max-subtracted (online) log-sum-exp, lanes strided over the columns, the lanes joined by an xor
//           butterfly.  Points live in LDS (three arrays, lane-strided reads: no bank conflict); the cost comes from coordinate
//           DIFFERENCES.  Launched as  INIT (sinkhorn_loop's initialisation at eps_s[0]),  SINKDIV_MAX_STEPS times as STEP (step s
//           returns at once when s >= n; Jacobi: reads buffer s & 1, writes the averaged potentials into the other) and once as
//           FINAL (the last extrapolation, no averaging; the softmax-weighted differences of the same pass give the gradient).
//   reduce  one wavefront: loss = mean(b_x - a_x) + mean(a_y - b_y), lane-strided float64 sums joined by wave_add's butterfly.
// Kernel boundaries order the iterations: no inter-workgroup waiting anywhere.  No float atomics: the same inputs give the same
// bits on every run.  Device memory is written by plain vector stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "moda_hip.h"
#include "moda_dev.h"

namespace {

constexpr int kMaxSteps = MODA_SINKDIV_MAX_STEPS;
constexpr int kMaxPoints = MODA_SINKDIV_MAX_POINTS;
constexpr int kHdrWords = 32;                  // [0] n (0 when flagged), [1] status flags, [2] d (float), [4 .. 4 + 24) eps (float)
constexpr int kRowsPerBlock = 8;               // 4 wavefronts, two rows each

struct Box { float lo[3], hi[3]; };

// ---- prep ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sinkdiv_prep_kernel(const float* __restrict__ x, const float* __restrict__ y, int N, int M,
                                                           double blur, double scaling, float diameter, int* __restrict__ hdr,
                                                           int* __restrict__ status) {
    __shared__ float sh[4][6];
    const int T = N + M, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float d = diameter;
    {   // the box pass runs with `diameter` given too: it is what sees a NaN or infinite coordinate
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        bool bad = false;
        for (int p = threadIdx.x; p < T; p += 256) {
            const float* q = p < N ? x + 3 * (long long)p : y + 3 * (long long)(p - N);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = q[c];
                bad = bad || !(fabsf(v) <= 3.4028235e38f);       // NaN or infinite coordinate
                lo[c] = fminf(lo[c], v);
                hi[c] = fmaxf(hi[c], v);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (bad) hi[c] = NAN;                                // fmaxf drops a NaN: carry it by hand
            lo[c] = wave_all(lo[c], [](float a, float b) { return fminf(a, b); });
            hi[c] = wave_all(hi[c], [](float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); });
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { sh[wave][c] = lo[c]; sh[wave][3 + c] = hi[c]; }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int c = 0; c < 3; ++c) {
                float l = sh[0][c], h = sh[0][3 + c];
                for (int w = 1; w < 4; ++w) {
                    l = fminf(l, sh[w][c]);
                    h = (h != h || sh[w][3 + c] != sh[w][3 + c]) ? NAN : fmaxf(h, sh[w][3 + c]);
                }
                const float e = h - l;                            // fp32, as the reference's (maxs - mins)
                s += (double)e * (double)e;
            }
            const float box = (float)sqrt(s);                     // NaN with a non-finite coordinate
            d = diameter > 0.f ? (box != box ? NAN : diameter) : box;
        }
    }
    if (threadIdx.x != 0) return;
    float* hdr_f = reinterpret_cast<float*>(hdr);
    int flags = 0, n = 0;
    const double dd = (double)d;
    if (!(dd <= 1.7e308) || !(dd > blur)) {
        flags |= MODA_SINKDIV_BAD_DIAMETER;                      // a non-finite coordinate, or arange(2 ln d, 2 ln blur, ..) is empty or undefined
    } else {
        const double start = 2.0 * log(dd), stop = 2.0 * log(blur), step = 2.0 * log(scaling);
        const double cnt = ceil((stop - start) / step);         // numpy's arange length
        if (!(cnt >= 1.0) || cnt + 2.0 > (double)kMaxSteps) {
            flags |= cnt >= 1.0 ? MODA_SINKDIV_TOO_MANY_STEPS : MODA_SINKDIV_BAD_DIAMETER;
        } else {
            n = (int)cnt + 2;
            hdr_f[4] = (float)(dd * dd);
            for (int k = 0; k < n - 2; ++k) hdr_f[5 + k] = (float)exp(start + (double)k * step);
            hdr_f[4 + n - 1] = (float)(blur * blur);
        }
    }
    hdr[0] = flags ? 0 : n;
    hdr[1] = flags;
    hdr_f[2] = d;
    status[0] = flags;
    status[1] = n;                                               // (0 when a flag is set)
    status[2] = __float_as_int(d);
    status[3] = 0;
}

// ---- rows ----------------------------------------------------------------------------------------------------------------
// running log-sum-exp of one lane: sum_k exp(v_k) = s * exp(m); g = sum_k exp(v_k - m) * (row - column)
struct Lse { float m, s, gx, gy, gz; };

template <bool GRAD>
DEVINL void lse_merge(Lse& a, const Lse& b) {
    const float mm = fmaxf(a.m, b.m);
    const float ea = a.m == mm ? 1.f : expf(a.m - mm), eb = b.m == mm ? 1.f : expf(b.m - mm);   // (an empty lane: m = -inf, s = 0)
    a.s = a.s * ea + b.s * eb;
    if (GRAD) { a.gx = a.gx * ea + b.gx * eb; a.gy = a.gy * ea + b.gy * eb; a.gz = a.gz * ea + b.gz * eb; }
    a.m = mm;
}

// softmin(eps, C, h)_r = -eps * logsumexp_k(h_k - C_rk / eps) over the columns [c0, c0 + cn) of the joined cloud, h_k = logw +
// pot[k] / eps (pot == nullptr: h_k = logw, the initialisation).  Every lane returns the whole row's value; g = the softmax-
// weighted sum of (row point - column point).  All 64 lanes call it together.
template <bool GRAD>
DEVINL float row_softmin(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz, int c0, int cn,
                         const float* __restrict__ pot, float logw, float eps, float rx, float ry, float rz, int lane, float g[3]) {
    Lse a{-INFINITY, 0.f, 0.f, 0.f, 0.f};
    for (int k = c0 + lane; k < c0 + cn; k += 64) {
        const float dx = rx - px[k], dy = ry - py[k], dz = rz - pz[k];
        const float C = (dx * dx + dy * dy + dz * dz) * 0.5f;
        const float h = pot ? logw + pot[k] / eps : logw;
        const float v = h - C / eps;
        const float e = expf(-fabsf(v - a.m));                    // one exponential per entry: the smaller of the two over the larger
        if (v > a.m) {
            a.s = a.s * e + 1.f;
            if (GRAD) { a.gx = a.gx * e + dx; a.gy = a.gy * e + dy; a.gz = a.gz * e + dz; }
            a.m = v;
        } else {
            a.s += e;
            if (GRAD) { a.gx += e * dx; a.gy += e * dy; a.gz += e * dz; }
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        Lse b;
        b.m = __shfl_xor(a.m, o, 64);
        b.s = __shfl_xor(a.s, o, 64);
        if (GRAD) { b.gx = __shfl_xor(a.gx, o, 64); b.gy = __shfl_xor(a.gy, o, 64); b.gz = __shfl_xor(a.gz, o, 64); }
        else { b.gx = b.gy = b.gz = 0.f; }
        lse_merge<GRAD>(a, b);
    }
    if (GRAD) { g[0] = a.gx / a.s; g[1] = a.gy / a.s; g[2] = a.gz / a.s; }
    return -eps * (a.m + logf(a.s));
}

enum { kInit = 0, kStep = 1, kFinal = 2 };

// pot: two buffers of 2 T floats, each [f (T), g (T)]: f_r = the softmin of point r over the x columns, g_r = over the y columns,
// i.e. (f, g) = (a_x, b_x) on the x rows and (a_y, b_y) on the y rows.  The update of f reads a_x on an x row and b_x on a y row
// -- the x-column entries of the ROW's own half: f for r < N, g otherwise -- and the update of g likewise reads the y-column
// entries of f (a_y) on an x row, of g (b_y) on a y row.
template <int MODE>
__global__ __launch_bounds__(256) void sinkdiv_rows_kernel(const float* __restrict__ x, const float* __restrict__ y, int N, int M,
                                                           float logwx, float logwy, int step, int* __restrict__ hdr,
                                                           float* __restrict__ pot, float* __restrict__ diff,
                                                           float* __restrict__ grad_x, float* __restrict__ grad_y) {
    extern __shared__ __attribute__((aligned(16))) float sh_pts[];
    const int T = N + M;
    const int n = hdr[0];                                         // 0: flagged by prep
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (MODE == kStep && step >= n) return;                       // (the whole grid: n is one word for everybody)
    if (n < 1) {
        if (MODE == kFinal) {                                     // flagged: zero gradients, nothing else is touched
            for (int r = blockIdx.x * kRowsPerBlock + wave; r < min(T, (int)(blockIdx.x + 1) * kRowsPerBlock); r += 4) {
                float* gr = r < N ? grad_x + 3 * (long long)r : (grad_y ? grad_y + 3 * (long long)(r - N) : nullptr);
                if (gr && lane < 3) gr[lane] = 0.f;
            }
        }
        return;
    }
    float* px = sh_pts;
    float* py = sh_pts + T;
    float* pz = sh_pts + 2 * T;
    for (int i = threadIdx.x; i < 3 * T; i += 256) {
        const float v = i < 3 * N ? x[i] : y[i - 3 * N];
        const int p = i / 3, c = i - 3 * p;
        sh_pts[c * T + p] = v;
    }
    __syncthreads();
    const float* hdr_f = reinterpret_cast<const float*>(hdr);
    const int s = MODE == kInit ? 0 : (MODE == kStep ? step : n - 1);
    const float eps = hdr_f[4 + s];
    // INIT writes buffer 0; STEP s reads buffer s & 1 and writes the other; FINAL reads buffer n & 1 and writes potentials nowhere
    const float* cur = pot + (long long)((MODE == kStep ? step : n) & 1) * 2 * T;
    float* nxt = pot + (long long)(MODE == kInit ? 0 : ((step + 1) & 1)) * 2 * T;
    const int r_end = min(T, (int)(blockIdx.x + 1) * kRowsPerBlock);
    for (int r = blockIdx.x * kRowsPerBlock + wave; r < r_end; r += 4) {      // (wave-uniform)
        const float rx = px[r], ry = py[r], rz = pz[r];
        const float* src = MODE == kInit ? nullptr : (r < N ? cur : cur + T);
        float gf[3], gg[3];
        const float tf = row_softmin<MODE == kFinal>(px, py, pz, 0, N, src, logwx, eps, rx, ry, rz, lane, gf);
        const float tg = row_softmin<MODE == kFinal>(px, py, pz, N, M, src, logwy, eps, rx, ry, rz, lane, gg);
        if (MODE == kInit) {
            if (lane == 0) { nxt[r] = tf; nxt[T + r] = tg; }
        } else if (MODE == kStep) {
            if (lane == 0) { nxt[r] = 0.5f * (cur[r] + tf); nxt[T + r] = 0.5f * (cur[T + r] + tg); }
        } else {
            // loss = sum_i alpha_i (b_x - a_x)_i + sum_j beta_j (a_y - b_y)_j; the envelope gradient through the row point
            const bool is_x = r < N;
            if (lane == 0) diff[r] = is_x ? tg - tf : tf - tg;
            float* gr = is_x ? grad_x + 3 * (long long)r : (grad_y ? grad_y + 3 * (long long)(r - N) : nullptr);
            if (gr && lane < 3) {
                const float w = is_x ? 1.f / (float)N : 1.f / (float)M;
                const float a = lane == 0 ? gf[0] : (lane == 1 ? gf[1] : gf[2]), b = lane == 0 ? gg[0] : (lane == 1 ? gg[1] : gg[2]);
                gr[lane] = w * (is_x ? b - a : a - b);
            }
        }
    }
}

// ---- reduce --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void sinkdiv_reduce_kernel(const int* __restrict__ hdr, const float* __restrict__ diff, int N, int M,
                                                            float* __restrict__ loss) {
    if (hdr[0] < 1) {
        if (threadIdx.x == 0) loss[0] = NAN;
        return;
    }
    double sx = 0.0, sy = 0.0;
    for (int i = threadIdx.x; i < N; i += 64) sx += (double)diff[i];
    for (int j = threadIdx.x; j < M; j += 64) sy += (double)diff[N + j];
    sx = wave_add(sx);
    sy = wave_add(sy);
    if (threadIdx.x == 0) loss[0] = (float)(sx / (double)N + sy / (double)M);
}

}  // namespace

extern "C" int64_t moda_sinkdiv_ws_bytes(int64_t N, int64_t M) {
    if (N < 1 || M < 1 || N + M > kMaxPoints) return 0;
    return 4 * (kHdrWords + 5 * (N + M));                         // header, two buffers of 2 (N + M) potentials, (N + M) row terms
}

extern "C" int moda_sinkdiv(const float* x, const float* y, int64_t N, int64_t M, double blur, double scaling, double diameter, void* ws,
                            float* loss_out, float* grad_x, float* grad_y, int32_t* status, void* stream) {
    if (!x || !y || !ws || !loss_out || !grad_x || !status) return MODA_EINVAL;
    if (N < 1 || M < 1 || !(blur > 0.0) || !(scaling > 0.0 && scaling < 1.0) || ((uintptr_t)ws & 3)) return MODA_EINVAL;
    if (N + M > kMaxPoints) return MODA_ESHAPE;
    const int n = (int)N, m = (int)M, T = n + m;
    int* hdr = (int*)ws;
    float* pot = (float*)ws + kHdrWords;
    float* diff = pot + 4 * (long long)T;
    const float logwx = logf(1.f / (float)n), logwy = logf(1.f / (float)m);       // ln alpha_i, ln beta_j of uniform weights
    const float dgiven = diameter > 0.0 ? (float)diameter : 0.f;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((T + kRowsPerBlock - 1) / kRowsPerBlock)), block(256);
    const size_t lds = (size_t)3 * T * sizeof(float);                            // <= 48 KB
    hipLaunchKernelGGL(sinkdiv_prep_kernel, dim3(1), dim3(256), 0, st, x, y, n, m, blur, scaling, dgiven, hdr, status);
    hipLaunchKernelGGL(sinkdiv_rows_kernel<kInit>, grid, block, lds, st, x, y, n, m, logwx, logwy, 0, hdr, pot, diff, grad_x, grad_y);
    for (int s = 0; s < kMaxSteps; ++s)
        hipLaunchKernelGGL(sinkdiv_rows_kernel<kStep>, grid, block, lds, st, x, y, n, m, logwx, logwy, s, hdr, pot, diff, grad_x, grad_y);
    hipLaunchKernelGGL(sinkdiv_rows_kernel<kFinal>, grid, block, lds, st, x, y, n, m, logwx, logwy, 0, hdr, pot, diff, grad_x, grad_y);
    hipLaunchKernelGGL(sinkdiv_reduce_kernel, dim3(1), dim3(64), 0, st, (const int*)hdr, (const float*)diff, n, m, loss_out);
    return (int)hipGetLastError();
}
