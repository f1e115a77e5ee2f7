// Bone re-initialisation and surface sampling on the extracted rest mesh (reference nnutils/geom_utils.py:857-903 reinit_bones,
// which runs kmeans_pytorch over the mesh vertices, and nnutils/moda.py:687-692, pytorch3d.ops.sample_points_from_meshes).
// VALU- and launch-bound: no MFMA.
//
//   k-means     one Lloyd iteration is two launches.
//     assign    the K <= 64 centres sit in LDS as three planes padded with +inf to a multiple of four; every lane reads the SAME
//               four centres with one 16-byte read per plane (a uniform address: a broadcast) and keeps the nearest under a
//               strict <, in index order: lowest index among equal distances.  d = fma(dz, dz, fma(dy, dy, dx * dx)), every
//               operation rounded on its own in fp32 (contraction is off for this file), as in pointset_kernels.hip.
//               Sums: a wave handles 64 points at a time; for each cluster present in the batch (ballot) the members' x, y, z
//               are widened to float64 and added over the wave by wave_add's butterfly (__shfl_xor 32..1, non-members contribute 0),
//               the count is the ballot's popcount, and lane k adds the batch's result to ITS registers: lane k of a wave
//               owns cluster k.  Batches follow in index order, the four waves are added in wave order through LDS, the
//               workgroups (at most MODA_KMEANS_MAX_BLOCKS, grid-stride) write partials (blocks, K, 4).  No float atomics: for
//               given inputs the tree is fixed, so the bits are the same on every run.
//     finalise  one workgroup adds the partials in block order, forms centre = float64 sum / count rounded to fp32 once,
//               fills an empty cluster with the point the splitmix64 rule names, adds the K centre moves in index order
//               (float64), advances the iteration counter and sets `done`.  Both kernels return at once when `done` is set, so
//               the host enqueues several iterations and reads the flag back once.
//   sampling    face areas in fp32 (faces with an index outside [0, V) are counted, given area 0 and never read through), an
//               inclusive float64 prefix sum of the areas (tile sums, one workgroup scanning the tile sums, tile scans: the
//               structure of mesh_kernels.hip on the same block_scan, no atomics), then one lane per sample: binary search for the first face whose
//               CDF exceeds u0 * total, and the point at pytorch3d's barycentrics.
// Device memory is written only by plain vector stores and HIP atomic functions.  Indices are int32; offsets in 64 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kMaxK = MODA_KMEANS_MAX_K;
constexpr int kMaxBlocks = MODA_KMEANS_MAX_BLOCKS;
constexpr int kPerThread = 8;
constexpr int kTile = kBlock * kPerThread;           // MODA_MC_SCAN_TILE
static_assert(kTile == MODA_MC_SCAN_TILE, "scan tile");
static_assert(4 * kMaxK <= kBlock && kMaxK <= 64, "one lane per cluster, one thread per (cluster, sum)");

DEVINL float dist2_1(float qx, float qy, float qz, float tx, float ty, float tz) {
    const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
    float d = dx * dx;
    d = __builtin_fmaf(dy, dy, d);
    return __builtin_fmaf(dz, dz, d);
}

// state[0] = iterations done, state[1] = done flag
__global__ __launch_bounds__(kBlock) void kmeans_assign_kernel(const float* __restrict__ x, int N, int K,
                                                               const float* __restrict__ centers, const int* __restrict__ state,
                                                               int* __restrict__ assign, double* __restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float c[3][kMaxK];
    __shared__ double red[kWaves][kMaxK][4];
    if (state[1]) return;                                                   // uniform: the whole grid leaves
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t < kMaxK) {
        const bool in = t < K;                                              // padding: +inf, whose distance never wins
        c[0][t] = in ? centers[3 * t + 0] : __builtin_inff();
        c[1][t] = in ? centers[3 * t + 1] : __builtin_inff();
        c[2][t] = in ? centers[3 * t + 2] : __builtin_inff();
    }
    __syncthreads();
    const int K4 = (K + 3) & ~3;
    double ax = 0.0, ay = 0.0, az = 0.0;                                    // lane k: the sums of cluster k in this wave
    int cnt = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int nbatch = (int)((N + stride - 1) / stride);                    // the same for every lane: the shuffles below
    for (int it = 0; it < nbatch; ++it) {
        const int64_t i = it * stride + (int64_t)blockIdx.x * kBlock + t;
        const bool valid = i < N;
        float px = 0.f, py = 0.f, pz = 0.f;
        if (valid) {
            px = x[i * 3 + 0];
            py = x[i * 3 + 1];
            pz = x[i * 3 + 2];
        }
        float best = __builtin_inff();
        int bi = 0;                                                         // stays 0 when nothing is finite and ordered
        for (int j = 0; j < K4; j += 4) {
            const float4 tx = *reinterpret_cast<const float4*>(&c[0][j]);
            const float4 ty = *reinterpret_cast<const float4*>(&c[1][j]);
            const float4 tz = *reinterpret_cast<const float4*>(&c[2][j]);
            const float d0 = dist2_1(px, py, pz, tx.x, ty.x, tz.x), d1 = dist2_1(px, py, pz, tx.y, ty.y, tz.y);
            const float d2 = dist2_1(px, py, pz, tx.z, ty.z, tz.z), d3 = dist2_1(px, py, pz, tx.w, ty.w, tz.w);
            if (d0 < best) { best = d0; bi = j; }
            if (d1 < best) { best = d1; bi = j + 1; }
            if (d2 < best) { best = d2; bi = j + 2; }
            if (d3 < best) { best = d3; bi = j + 3; }
        }
        if (valid) assign[i] = bi;
        const int a = valid ? bi : -1;
        for (int k = 0; k < K; ++k) {
            const bool mine = a == k;
            const unsigned long long m = __ballot(mine);
            if (!m) continue;                                               // wave-uniform
            const double vx = wave_add(mine ? (double)px : 0.0), vy = wave_add(mine ? (double)py : 0.0),
                         vz = wave_add(mine ? (double)pz : 0.0);
            if (lane == k) {
                ax += vx;
                ay += vy;
                az += vz;
                cnt += __popcll(m);
            }
        }
    }
    if (lane < K) {
        red[w][lane][0] = ax;
        red[w][lane][1] = ay;
        red[w][lane][2] = az;
        red[w][lane][3] = (double)cnt;                                      // < 2^31: exact
    }
    __syncthreads();
    if (t < 4 * K) {
        const int k = t >> 2, q = t & 3;
        double v = 0.0;
#pragma unroll
        for (int ww = 0; ww < kWaves; ++ww) v += red[ww][k][q];
        partials[((int64_t)blockIdx.x * K + k) * 4 + q] = v;
    }
}

DEVINL unsigned long long splitmix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(kBlock) void kmeans_final_kernel(const float* __restrict__ x, int N, int K, int nblk,
                                                              const double* __restrict__ partials, float* __restrict__ centers,
                                                              int* __restrict__ counts, int* __restrict__ state,
                                                              double* __restrict__ shift, double tol, int iter_limit,
                                                              unsigned long long seed) {
    __shared__ double s[kMaxK][4];
    __shared__ double moved[kMaxK];
    if (state[1]) return;
    const int t = threadIdx.x;
    if (t < 4 * K) {
        double v = 0.0;
#pragma unroll 8
        for (int b = 0; b < nblk; ++b) v += partials[(int64_t)b * K * 4 + t];   // block order: the same bits on every run
        s[t >> 2][t & 3] = v;
    }
    const int iteration = state[0];
    __syncthreads();
    if (t < K) {
        const long long n = (long long)s[t][3];
        float nc[3];
        if (n > 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) nc[q] = (float)(s[t][q] / (double)n);
        } else {                                                            // empty: the point the rule names
            const unsigned long long z =
                splitmix64(seed + 0x9E3779B97F4A7C15ull * ((unsigned long long)iteration * (unsigned long long)K + (unsigned long long)t + 1ull));
            const int64_t p = (int64_t)(z % (unsigned long long)N);
#pragma unroll
            for (int q = 0; q < 3; ++q) nc[q] = x[p * 3 + q];
        }
        const double dx = (double)nc[0] - (double)centers[3 * t + 0];
        const double dy = (double)nc[1] - (double)centers[3 * t + 1];
        const double dz = (double)nc[2] - (double)centers[3 * t + 2];
        moved[t] = sqrt((dx * dx + dy * dy) + dz * dz);
#pragma unroll
        for (int q = 0; q < 3; ++q) centers[3 * t + q] = nc[q];
        counts[t] = (int)n;
    }
    __syncthreads();
    if (t == 0) {
        double sh = 0.0;
        for (int k = 0; k < K; ++k) sh += moved[k];
        const int it = iteration + 1;
        state[0] = it;
        *shift = sh;
        if (sh * sh < tol || (iter_limit != 0 && it >= iter_limit)) state[1] = 1;
    }
}

// ---- surface sampling ---------------------------------------------------------------------------------------------------
DEVINL bool face_ok(const int* faces, int64_t f, int nv) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    return a >= 0 && b >= 0 && c >= 0 && a < nv && b < nv && c < nv;
}

__global__ __launch_bounds__(kBlock) void face_area_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int V,
                                                           int F, float* __restrict__ areas, unsigned long long* __restrict__ n_bad) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= F) return;
    if (!face_ok(faces, f, V)) {
        areas[f] = 0.f;
        atomicAdd(n_bad, 1ull);
        return;
    }
    const float* a = verts + 3LL * faces[3LL * f];
    const float* b = verts + 3LL * faces[3LL * f + 1];
    const float* c = verts + 3LL * faces[3LL * f + 2];
    const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
    const float vx = c[0] - a[0], vy = c[1] - a[1], vz = c[2] - a[2];
    const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    areas[f] = 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
}

// the exclusive value of a block_scan: the earlier waves' sum first, then the wave's own earlier lanes -- this association is the CDF's
DEVINL double scan_exclusive(const BlockScan<double>& r) {
    const double prev = __shfl_up(r.incl_wave, 1);
    return (threadIdx.x & 63) == 0 ? r.before : r.before + prev;
}

__global__ __launch_bounds__(kBlock) void cdf_tile_sum_kernel(const float* __restrict__ areas, int n, double* __restrict__ tile_sum) {
    __shared__ double lds[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kTile + threadIdx.x * kPerThread;
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kPerThread; ++q)
        if (base + q < n) s += (double)areas[base + q];
    const BlockScan<double> r = block_scan<double, kWaves>(s, lds);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = r.total;
}

// one block: exclusive scan of the tile sums
__global__ __launch_bounds__(1024) void cdf_tiles_kernel(const double* __restrict__ tile_sum, int nt, double* __restrict__ tile_off) {
    __shared__ double lds[1024 / 64];
    double carry = 0.0;
    for (int b0 = 0; b0 < nt; b0 += 1024) {
        const int b = b0 + (int)threadIdx.x;
        const BlockScan<double> r = block_scan<double, 1024 / 64>(b < nt ? tile_sum[b] : 0.0, lds);
        const double excl = scan_exclusive(r);
        if (b < nt) tile_off[b] = carry + excl;
        carry += r.total;
    }
}

__global__ __launch_bounds__(kBlock) void cdf_tile_kernel(const float* __restrict__ areas, int n, const double* __restrict__ tile_off,
                                                          double* __restrict__ cdf) {
    __shared__ double lds[kWaves];
    const int64_t base = (int64_t)blockIdx.x * kTile + threadIdx.x * kPerThread;
    double c[kPerThread];
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
        c[q] = base + q < n ? (double)areas[base + q] : 0.0;
        s += c[q];
    }
    double run = tile_off[blockIdx.x] + scan_exclusive(block_scan<double, kWaves>(s, lds));
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
        run += c[q];
        if (base + q < n) cdf[base + q] = run;                              // inclusive
    }
}

__global__ __launch_bounds__(kBlock) void sample_draw_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int V,
                                                             int F, const float* __restrict__ areas, const double* __restrict__ cdf,
                                                             const float* __restrict__ u, int S, float* __restrict__ points,
                                                             int* __restrict__ face_idx) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= S) return;
    const float u0 = u[3LL * i], u1 = u[3LL * i + 1], u2 = u[3LL * i + 2];
    const double target = (double)u0 * cdf[F - 1];
    int lo = 0, hi = F - 1;                                                 // the first face whose CDF exceeds the target
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > target) hi = mid;
        else lo = mid + 1;
    }
    // The scan's sums are rounded, so across a thread boundary of the scan the CDF of a zero-area face can differ from its
    // predecessor's in the last bit; such a face is stepped over: a face of area 0 is never the answer.
    int f = lo;
    while (f + 1 < F && !(areas[f] > 0.f)) ++f;
    while (f > 0 && !(areas[f] > 0.f)) --f;
    float* o = points + 3LL * i;
    if (!face_ok(faces, f, V)) {                                            // never read through a bad face
        o[0] = o[1] = o[2] = __builtin_nanf("");
        face_idx[i] = -1;
        return;
    }
    const float* a = verts + 3LL * faces[3LL * f];
    const float* b = verts + 3LL * faces[3LL * f + 1];
    const float* c = verts + 3LL * faces[3LL * f + 2];
    const float s = sqrtf(u1);
    const float w0 = 1.0f - s, w1 = s * (1.0f - u2), w2 = s * u2;
#pragma unroll
    for (int d = 0; d < 3; ++d) o[d] = __builtin_fmaf(w2, c[d], __builtin_fmaf(w1, b[d], w0 * a[d]));
    face_idx[i] = f;
}

}   // namespace

extern "C" int32_t moda_kmeans_blocks(int64_t N) {
    if (N < 1) return 0;
    const int64_t b = (N + kBlock - 1) / kBlock;
    return (int32_t)(b < kMaxBlocks ? b : kMaxBlocks);
}

extern "C" int moda_kmeans_steps(const float* x, int64_t N, int32_t K, float* centers, int32_t* assign, double* partials,
                                 int32_t* counts, int32_t* state, double* shift, double tol, int32_t iter_limit, uint64_t seed,
                                 int32_t steps, void* stream) {
    if (K < 1 || K > kMaxK || steps < 0 || iter_limit < 0) return MODA_EINVAL;
    if (N < K || N >= 2147483648LL) return MODA_ESHAPE;
    if (!x || !centers || !assign || !partials || !counts || !state || !shift) return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = moda_kmeans_blocks(N);
    for (int s = 0; s < steps; ++s) {
        hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)nblk), dim3(kBlock), 0, st, x, (int)N, (int)K, (const float*)centers,
                           (const int*)state, assign, partials);
        hipLaunchKernelGGL(kmeans_final_kernel, dim3(1), dim3(kBlock), 0, st, x, (int)N, (int)K, nblk, (const double*)partials,
                           centers, counts, state, shift, tol, (int)iter_limit, (unsigned long long)seed);
    }
    return (int)hipGetLastError();
}

extern "C" int moda_mesh_face_cdf(const float* verts, const int32_t* faces, int64_t V, int64_t F, float* areas, double* cdf,
                                  double* tile_sum, double* tile_off, int64_t* n_bad, void* stream) {
    if (V < 1 || F < 1 || V >= 2147483648LL || 3 * F >= 2147483648LL) return MODA_ESHAPE;
    if (!verts || !faces || !areas || !cdf || !tile_sum || !tile_off || !n_bad) return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(n_bad, 0, sizeof(int64_t), st);
    if (e != hipSuccess) return (int)e;
    const int nf = (int)F;
    const unsigned nt = nblocks(F, kTile);
    hipLaunchKernelGGL(face_area_kernel, dim3(nblocks(F, kBlock)), dim3(kBlock), 0, st, verts, faces, (int)V, nf, areas,
                       (unsigned long long*)n_bad);
    hipLaunchKernelGGL(cdf_tile_sum_kernel, dim3(nt), dim3(kBlock), 0, st, (const float*)areas, nf, tile_sum);
    hipLaunchKernelGGL(cdf_tiles_kernel, dim3(1), dim3(1024), 0, st, (const double*)tile_sum, (int)nt, tile_off);
    hipLaunchKernelGGL(cdf_tile_kernel, dim3(nt), dim3(kBlock), 0, st, (const float*)areas, nf, (const double*)tile_off, cdf);
    return (int)hipGetLastError();
}

extern "C" int moda_mesh_sample(const float* verts, const int32_t* faces, int64_t V, int64_t F, const float* areas,
                                const double* cdf, const float* u, int64_t S, float* points, int32_t* face_idx, void* stream) {
    if (V < 1 || F < 1 || S < 0 || V >= 2147483648LL || 3 * F >= 2147483648LL || 3 * S >= 2147483648LL) return MODA_ESHAPE;
    if (S == 0) return 0;
    if (!verts || !faces || !areas || !cdf || !u || !points || !face_idx) return MODA_EINVAL;
    hipLaunchKernelGGL(sample_draw_kernel, dim3(nblocks(S, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, verts, faces, (int)V,
                       (int)F, areas, cdf, u, (int)S, points, face_idx);
    return (int)hipGetLastError();
}
