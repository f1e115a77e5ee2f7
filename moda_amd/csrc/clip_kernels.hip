// Per-group gradient clipping with NaN / inf rejection and stage freezing, device-resident (reference
// nnutils/train_utils.py:1154-1311 clip_grad: isnan scan, zero_grad_list of the frozen groups, 22 clip_grad_norm_ calls, zero
// everything when a NaN was seen).  Memory- and launch-bound: no MFMA.  Three launches, no host sync, no allocation.
//
//   tables     segments (pointer, numel, group, frozen byte) are the gradient tensors; a chunk is MODA_CLIP_CHUNK floats of ONE
//              segment (its last chunk is shorter), so chunk starts keep their segment's alignment.  Chunks are sorted by group:
//              group g owns chunks [group_begin[g], group_begin[g + 1]), the ungrouped ones follow group_begin[G].
//   partials   one workgroup per chunk.  Lane t owns the quads t, t + 256, t + 512, t + 768 of the chunk -- one float4 load each
//              where the segment's base is 16-byte aligned, four bounds-checked scalar loads otherwise and in the tail quad, the
//              SAME element-to-lane map either way, so a norm does not depend on where its tensors lie.  Each square is rounded
//              in fp32 (contraction is off for this file), widened to float64 and added in element order per lane, over the wave
//              by wave_add's butterfly (__shfl_xor 32..1), over the four waves in wave order through LDS.  NaN and +-inf elements are
//              counted separately.  A frozen chunk (its group's byte or its segment's) is scanned for non-finite values like any
//              other -- the reference tests for NaN before it freezes -- but contributes 0 to the sum.
//   finalize   one workgroup.  Wave w takes groups w, w + 4, ...: the group's partials are added strictly in table order (64 are
//              loaded at a time, one per lane, and broadcast in turn), norm = (float)sqrt(sum), coef = min(1, max / (norm + 1e-6))
//              in the fp32 operations torch's clip_grad_norm_ performs; a frozen group reports norm 0 and coef 0.
//   apply      one workgroup per chunk: literal zeros when the step is invalid or the chunk is frozen (NaN * 0 is NaN, so no
//              product), nothing when the chunk is ungrouped or coef == 1, else g * coef rounded once.
// No float atomics: for given inputs every sum has one fixed tree, so the bits are the same on every run.
// Device memory is written only by plain vector stores.  Chunk and segment indices are int32; element offsets in 64 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = MODA_CLIP_CHUNK;
constexpr int kQuads = kChunk / 4 / kBlock;          // quads per lane
static_assert(kQuads * 4 * kBlock == kChunk, "a chunk is a whole number of quads per lane");

struct Tables {
    float* const* seg_ptr;
    const int64_t* seg_numel;
    const int32_t* seg_group;
    const uint8_t* seg_frozen;
    int32_t n_seg;
    const int32_t* chunk_seg;
    const int64_t* chunk_off;
    int32_t G;
    const uint8_t* frozen;
};

struct Chunk {
    float* p;        // first element
    int n;           // 1..kChunk elements, 0: a table entry the kernels refuse to follow
    int group;       // -1: ungrouped
    bool frozen, aligned;
};

DEVINL Chunk chunk_of(const Tables& T, int c) {
    Chunk k{nullptr, 0, -1, false, false};
    const int s = T.chunk_seg[c];
    if (s < 0 || s >= T.n_seg) return k;
    const int64_t numel = T.seg_numel[s], off = T.chunk_off[c];
    const int g = T.seg_group[s];
    float* base = T.seg_ptr[s];
    if (!base || off < 0 || off >= numel || g < -1 || g >= T.G) return k;
    k.p = base + off;
    k.n = (int)(numel - off < (int64_t)kChunk ? numel - off : (int64_t)kChunk);
    k.group = g;
    k.frozen = T.seg_frozen[s] != 0 || (g >= 0 && T.frozen[g] != 0);
    k.aligned = ((uintptr_t)k.p & 15) == 0;
    return k;
}

// quad q of a chunk: v[0..cnt), cnt = the elements of the quad inside the chunk
DEVINL int load_quad(const Chunk& k, int q, float v[4]) {
    const int e = 4 * q;
    if (k.aligned && e + 4 <= k.n) {
        const float4 t = *reinterpret_cast<const float4*>(k.p + e);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        return 4;
    }
    const int cnt = k.n - e < 4 ? (k.n - e > 0 ? k.n - e : 0) : 4;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < cnt) v[j] = k.p[e + j];
    return cnt;
}

DEVINL void store_quad(const Chunk& k, int q, const float v[4]) {
    const int e = 4 * q;
    if (k.aligned && e + 4 <= k.n) {
        *reinterpret_cast<float4*>(k.p + e) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (e + j < k.n) k.p[e + j] = v[j];
}

__global__ __launch_bounds__(kBlock) void clip_partial_kernel(Tables T, double* __restrict__ partial, int32_t* __restrict__ nonfinite) {
    __shared__ double red[kWaves];
    __shared__ int red_n[kWaves][2];
    const int c = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const Chunk k = chunk_of(T, c);
    double acc = 0.0;
    int n_nan = 0, n_inf = 0;
#pragma unroll
    for (int i = 0; i < kQuads; ++i) {
        float v[4];
        const int cnt = load_quad(k, t + kBlock * i, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= cnt) break;
            n_nan += v[j] != v[j];
            n_inf += __builtin_isinf(v[j]) ? 1 : 0;
            const float sq = v[j] * v[j];
            if (!k.frozen) acc += (double)sq;
        }
    }
    acc = wave_add(acc);
    n_nan = wave_add(n_nan);
    n_inf = wave_add(n_inf);
    if (lane == 0) {
        red[w] = acc;
        red_n[w][0] = n_nan;
        red_n[w][1] = n_inf;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        int a = 0, b = 0;
#pragma unroll
        for (int ww = 0; ww < kWaves; ++ww) {
            s += red[ww];
            a += red_n[ww][0];
            b += red_n[ww][1];
        }
        partial[c] = s;
        nonfinite[2 * c] = a;
        nonfinite[2 * c + 1] = b;
    }
}

__global__ __launch_bounds__(kBlock) void clip_finalize_kernel(const double* __restrict__ partial, const int32_t* __restrict__ nonfinite,
                                                               int n_chunks, const int32_t* __restrict__ group_begin, int G,
                                                               const float* __restrict__ max_norm, const uint8_t* __restrict__ frozen,
                                                               float* __restrict__ coef, float* __restrict__ norms,
                                                               int32_t* __restrict__ status) {
    __shared__ long long red_n[kWaves][2];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    long long n_nan = 0, n_inf = 0;                                          // integers: any order gives the same total
    for (int c = t; c < n_chunks; c += kBlock) {
        n_nan += nonfinite[2 * c];
        n_inf += nonfinite[2 * c + 1];
    }
    n_nan = wave_add(n_nan);
    n_inf = wave_add(n_inf);
    if (lane == 0) {
        red_n[w][0] = n_nan;
        red_n[w][1] = n_inf;
    }
    for (int g = w; g < G; g += kWaves) {                                    // wave-uniform
        int b = group_begin[g], e = group_begin[g + 1];
        b = b < 0 ? 0 : (b > n_chunks ? n_chunks : b);
        e = e < b ? b : (e > n_chunks ? n_chunks : e);
        double s = 0.0;                                                      // the same in every lane
        for (int base = b; base < e; base += 64) {
            const double v = base + lane < e ? partial[base + lane] : 0.0;
            const int m = e - base < 64 ? e - base : 64;
            for (int j = 0; j < m; ++j) s += __shfl(v, j);                   // table order
        }
        if (lane == 0) {
            const bool fz = frozen[g] != 0;
            const float norm = fz ? 0.f : (float)sqrt(s);
            norms[g] = norm;
            coef[g] = fz ? 0.f : fminf(1.f, __fdiv_rn(max_norm[g], __fadd_rn(norm, 1e-6f)));
        }
    }
    __syncthreads();
    if (t == 0) {
        long long a = 0, b = 0;
#pragma unroll
        for (int ww = 0; ww < kWaves; ++ww) {
            a += red_n[ww][0];
            b += red_n[ww][1];
        }
        status[0] = (a | b) != 0;
        status[1] = (int32_t)(a > 2147483647LL ? 2147483647LL : a);
        status[2] = (int32_t)(b > 2147483647LL ? 2147483647LL : b);
        status[3] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void clip_apply_kernel(Tables T, const float* __restrict__ coef, const int32_t* __restrict__ status) {
    const int c = blockIdx.x, t = threadIdx.x;
    const Chunk k = chunk_of(T, c);
    if (k.n == 0) return;
    const bool zero = status[0] != 0 || k.frozen;                            // block-uniform, like everything below
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (zero) {
#pragma unroll
        for (int i = 0; i < kQuads; ++i) store_quad(k, t + kBlock * i, v);
        return;
    }
    if (k.group < 0) return;
    const float cf = coef[k.group];
    if (cf == 1.f) return;
#pragma unroll
    for (int i = 0; i < kQuads; ++i) {
        const int cnt = load_quad(k, t + kBlock * i, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) v[j] = v[j] * cf;
        store_quad(k, t + kBlock * i, v);
    }
}

}   // namespace

extern "C" int moda_clip_grad(float* const* seg_ptr, const int64_t* seg_numel, const int32_t* seg_group, const uint8_t* seg_frozen,
                              int32_t n_seg, const int32_t* chunk_seg, const int64_t* chunk_off, int32_t n_chunks,
                              const int32_t* group_begin, int32_t G, const float* max_norm, const uint8_t* frozen, double* partial,
                              int32_t* nonfinite, float* coef, float* norms, int32_t* status, void* stream) {
    if (n_seg < 0 || n_chunks < 0 || G < 1) return MODA_EINVAL;
    if (!group_begin || !max_norm || !frozen || !coef || !norms || !status) return MODA_EINVAL;
    if (n_chunks > 0 && (!seg_ptr || !seg_numel || !seg_group || !seg_frozen || !chunk_seg || !chunk_off || !partial || !nonfinite
                         || n_seg < 1))
        return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Tables T{seg_ptr, seg_numel, seg_group, seg_frozen, n_seg, chunk_seg, chunk_off, G, frozen};
    if (n_chunks > 0)
        hipLaunchKernelGGL(clip_partial_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, st, T, partial, nonfinite);
    hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)partial, (const int32_t*)nonfinite,
                       (int)n_chunks, group_begin, (int)G, max_norm, frozen, coef, norms, status);
    if (n_chunks > 0)
        hipLaunchKernelGGL(clip_apply_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, st, T, (const float*)coef,
                           (const int32_t*)status);
    return (int)hipGetLastError();
}
