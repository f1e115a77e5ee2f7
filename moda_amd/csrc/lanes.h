// The small vocabulary every kernel file of libmoda_hip.so shares (moda_dev.h includes it; the files that need nothing else of
// moda_dev.h include it directly): DEVINL, the launch-size and alignment helpers of the entry points, the int32 / int64 index
// load, and the 64-lane wave reductions and scans with the workgroup scan built on them.  Each has ONE fixed tree, which the
// callers' headers name: nothing here multiplies, so floating-point contraction has nothing to change.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DEVINL __device__ __forceinline__

namespace {

inline unsigned nblocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

DEVINL long long load_id(const void* p, int is64, long long i) {
    return is64 ? (long long)((const int64_t*)p)[i] : (long long)((const int32_t*)p)[i];
}

// The wave helpers need all 64 lanes ACTIVE (call them in wave-uniform control flow).

// xor butterfly: v[l] = op(v[l], v[l ^ o]) for o = 32, 16, ..., 1; the result ends up in every lane
template <class T, class Op>
DEVINL T wave_all(T v, Op op) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}

template <class T>
DEVINL T wave_add(T v) {
    return wave_all(v, [](T a, T b) { return a + b; });
}

// `__shfl_down` tree: v[l] += v[l + o] for o = 32, 16, ..., 1; the result is valid in lane 0 only
template <class T>
DEVINL T wave_add_down(T v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// inclusive scan over the wave (Hillis-Steele): v[l] += v[l - o] for o = 1, 2, ..., 32 where lane l >= o
template <class T>
DEVINL T wave_scan_incl(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// Scan over a workgroup of WAVES waves (lds: WAVES values, reusable after the call's second barrier): incl_wave = the inclusive
// scan inside the caller's wave, before = the earlier waves' totals added in index order from zero, total = all waves' totals
// added in index order.  The caller forms its own result from the three, which is what fixes its association.
template <class T>
struct BlockScan { T incl_wave, before, total; };

template <class T, int WAVES>
DEVINL BlockScan<T> block_scan(T v, T* lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    BlockScan<T> r;
    r.incl_wave = wave_scan_incl(v, lane);
    if (lane == 63) lds[wave] = r.incl_wave;
    __syncthreads();
    r.before = 0;
    r.total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const T t = lds[w];
        if (w < wave) r.before += t;
        r.total += t;
    }
    __syncthreads();
    return r;
}

}   // namespace
