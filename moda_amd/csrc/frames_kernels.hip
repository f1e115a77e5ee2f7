// The per-frame tables of a training run on the device (reference nnutils/moda.py:1497-1513, banmo.save_latest_vars; :485-491, the
// near-far reset of forward_default; nnutils/geom_utils.py:1105-1155, get_near_far over pts_to_view): the scatter of a batch's
// poses into the tables by frame id, and the near / far planes of every seen frame from the depth range of a point set,
// optionally fused with the pose patch that precedes it.  Nothing allocates, synchronises or reads back; every launch goes to
// the caller's stream.  No float atomics (the only atomics are integer counts of NaN frames and refused ids): min and max do
// not depend on the order their operands arrive in, and a table row has exactly one writer, so the bits are the same on every
// run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;               // the block kernel: four waves a (frame, point range)
constexpr int kWave = 64;
constexpr int kSmallBlock = 64;           // the small-N kernel and the scatter: one lane a frame / batch entry
constexpr int kSmallN = 32;               // up to this many points a frame is one lane's loop
constexpr int kMinPoints = 4096;          // a point range is never shorter than this (16 points a lane)
constexpr int kMaxSplit = MODA_NEAR_FAR_MAX_SPLIT;
constexpr long long kWantBlocks = 1024;   // 4 workgroups on each of the 256 CUs before the points are split

// torch.clamp(v, min=lo): NaN stays NaN (fmaxf would drop it).
DEVINL float clamp_min(float v, float lo) { return v != v ? v : (v < lo ? lo : v); }

struct Pose {
    float r[3][3], t[3];
};

// The pose the planes of frame m are computed from: rtk_all[m] where the patch applies (rtk_all given and idk != 0, numpy's
// astype(bool): a NaN counts as seen), otherwise rows 0-2 of the table.  `store`: also write the patch into the table.
DEVINL void load_pose(Pose& p, float* __restrict__ tab_rtk, const float* __restrict__ rtk_all, long long m, bool patch, bool store) {
    const float* src = patch ? rtk_all + m * 12 : tab_rtk + m * 16;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) p.r[i][j] = src[i * 4 + j];
        p.t[i] = src[i * 4 + 3];
    }
    if (patch && store) {
#pragma unroll
        for (int i = 0; i < 12; ++i) tab_rtk[m * 16 + i] = src[i];
    }
}

// Depth of one point as pts_to_view forms it: obj_to_cam (p R^T + T), then pinhole_cam's product with K2mat's transpose, whose
// last column is (0, 0, 1): z' = x * 0 + y * 0 + z * 1.  For finite x and y that is z; an infinite or NaN x or y makes it NaN,
// as in the reference, which is why all three rows are evaluated.
DEVINL float depth(const Pose& p, float px, float py, float pz) {
    const float x = ((px * p.r[0][0] + py * p.r[0][1]) + pz * p.r[0][2]) + p.t[0];
    const float y = ((px * p.r[1][0] + py * p.r[1][1]) + pz * p.r[1][2]) + p.t[1];
    const float z = ((px * p.r[2][0] + py * p.r[2][1]) + pz * p.r[2][2]) + p.t[2];
    return (x * 0.f + y * 0.f) + z;
}

struct Range {
    float lo, hi;
    int nan;
};

DEVINL void take(Range& a, float z) {
    a.nan |= (z != z) ? 1 : 0;
    a.lo = fminf(a.lo, z);
    a.hi = fmaxf(a.hi, z);
}

// get_near_far's tail for one frame: delta, the two planes, the clamp, the write.  Called by the frame's single finishing lane.
DEVINL void finish(const Range& a, float fac, long long m, float* __restrict__ near_far, int* __restrict__ status) {
    const float nanv = __uint_as_float(0x7fc00000u);
    float nr = nanv, fr = nanv;
    if (!a.nan) {
        const float delta = (a.hi - a.lo) * fac;
        nr = clamp_min(a.lo - delta, 1e-3f);
        fr = clamp_min(a.hi + delta, 1e-3f);
    }
    if (nr != nr || fr != fr) atomicAdd(status, 1);
    near_far[m * 2] = nr;
    near_far[m * 2 + 1] = fr;
}

// N <= kSmallN (the per-step reset's 8 box corners): one lane a frame, the points read by every lane at one address.
__global__ void near_far_small_kernel(const float* __restrict__ pts, int n, float* __restrict__ tab_rtk, const float* __restrict__ idk,
                                      float* __restrict__ near_far, long long M, float fac, const float* __restrict__ rtk_all,
                                      int* __restrict__ status) {
    const long long m = (long long)blockIdx.x * kSmallBlock + threadIdx.x;
    if (m >= M) return;
    const float seen = idk[m];
    const bool patch = rtk_all != nullptr && seen != 0.f;
    if (!patch && seen != 1.f) return;
    Pose p;
    load_pose(p, tab_rtk, rtk_all, m, patch, true);
    if (seen != 1.f) return;
    Range a = {__uint_as_float(0x7f800000u), __uint_as_float(0xff800000u), 0};
    for (int i = 0; i < n; ++i) take(a, depth(p, pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]));
    finish(a, fac, m, near_far, status);
}

// Grid (M, splits): workgroup (m, s) takes points [s * per, min(N, (s + 1) * per)) of frame m, lanes striding them; the wave
// reduces by shuffles, the four waves meet in LDS.  splits == 1: lane 0 finishes the frame.  Otherwise it leaves
// (min, max, NaN flag) in ws[(m * splits + s) * 3 ..] for near_far_finish_kernel.  Only split 0 stores the pose patch; every
// split of a patched frame READS rtk_all, never the table row being written.
__global__ void near_far_block_kernel(const float* __restrict__ pts, long long N, long long per, float* __restrict__ tab_rtk,
                                      const float* __restrict__ idk, float* __restrict__ near_far, float fac,
                                      const float* __restrict__ rtk_all, float* __restrict__ ws, int* __restrict__ status) {
    __shared__ float sh_lo[kBlock / kWave], sh_hi[kBlock / kWave];
    __shared__ int sh_nan[kBlock / kWave];
    const long long m = blockIdx.x;
    const int s = blockIdx.y, splits = gridDim.y;
    const float seen = idk[m];
    const bool patch = rtk_all != nullptr && seen != 0.f;
    if (!patch && seen != 1.f) return;                       // (uniform over the workgroup: no barrier is skipped by a part of it)
    Pose p;
    load_pose(p, tab_rtk, rtk_all, m, patch, s == 0 && threadIdx.x == 0);
    if (seen != 1.f) return;
    const long long lo = (long long)s * per, hi = (lo + per < N) ? lo + per : N;
    Range a = {__uint_as_float(0x7f800000u), __uint_as_float(0xff800000u), 0};
    for (long long i = lo + threadIdx.x; i < hi; i += kBlock) take(a, depth(p, pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]));
    a.lo = wave_all(a.lo, [](float x, float y) { return fminf(x, y); });
    a.hi = wave_all(a.hi, [](float x, float y) { return fmaxf(x, y); });
    a.nan = wave_all(a.nan, [](int x, int y) { return x | y; });
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) {
        sh_lo[wave] = a.lo;
        sh_hi[wave] = a.hi;
        sh_nan[wave] = a.nan;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) {
        a.lo = fminf(a.lo, sh_lo[w]);
        a.hi = fmaxf(a.hi, sh_hi[w]);
        a.nan |= sh_nan[w];
    }
    if (splits == 1) {
        finish(a, fac, m, near_far, status);
    } else {
        float* o = ws + (m * splits + s) * 3;
        o[0] = a.lo;
        o[1] = a.hi;
        o[2] = a.nan ? 1.f : 0.f;
    }
}

// The second kernel of a split launch: one lane a frame folds its `splits` partials in split order and finishes the frame.
__global__ void near_far_finish_kernel(const float* __restrict__ ws, int splits, const float* __restrict__ idk,
                                       float* __restrict__ near_far, long long M, float fac, int* __restrict__ status) {
    const long long m = (long long)blockIdx.x * kSmallBlock + threadIdx.x;
    if (m >= M || idk[m] != 1.f) return;
    Range a = {__uint_as_float(0x7f800000u), __uint_as_float(0xff800000u), 0};
    for (int s = 0; s < splits; ++s) {
        const float* o = ws + (m * splits + s) * 3;
        a.lo = fminf(a.lo, o[0]);
        a.hi = fmaxf(a.hi, o[1]);
        a.nan |= o[2] != 0.f ? 1 : 0;
    }
    finish(a, fac, m, near_far, status);
}

// save_latest_vars: one lane a batch entry.  numpy's fancy assignment keeps the LAST occurrence of a repeated index, so entry b
// writes its frame's rows only if no later entry names the same frame: every row has one writer.
__global__ void frames_scatter_kernel(const float* __restrict__ rtk, const float* __restrict__ kaug, const float* __restrict__ rt_raw,
                                      const long long* __restrict__ frameid, int bs, float* __restrict__ tab_rtk,
                                      float* __restrict__ tab_rt_raw, float* __restrict__ tab_idk, long long M,
                                      int* __restrict__ status) {
    const int b = blockIdx.x * kSmallBlock + threadIdx.x;
    if (b >= bs) return;
    const long long f = frameid[b];
    if (f < 0 || f >= M) {
        atomicAdd(status + 1, 1);
        return;
    }
    for (int c = b + 1; c < bs; ++c)
        if (frameid[c] == f) return;
    const float* src = rtk + (long long)b * 16;
    float* dst = tab_rtk + f * 16;
#pragma unroll
    for (int i = 0; i < 12; ++i) dst[i] = src[i];
    // mat2K(K2inv(kaug) @ K2mat(rtk[3])) in the reference's operations: the quotients of K2inv first, then the dot products of
    // the 3x3 product with their zero terms, summed left to right
    const float fx = src[12], fy = src[13], px = src[14], py = src[15];
    const float* ka = kaug + (long long)b * 4;
    const float a = 1.f / ka[0], bb = 1.f / ka[1], c = -ka[2] / ka[0], d = -ka[3] / ka[1];
    dst[12] = (a * fx + 0.f * 0.f) + c * 0.f;
    dst[13] = (0.f * 0.f + bb * fy) + d * 0.f;
    dst[14] = (a * px + 0.f * py) + c * 1.f;
    dst[15] = (0.f * px + bb * py) + d * 1.f;
    const float* rs = rt_raw + (long long)b * 12;
    float* rd = tab_rt_raw + f * 12;
#pragma unroll
    for (int i = 0; i < 12; ++i) rd[i] = rs[i];
    tab_idk[f] = 1.f;
}

inline int auto_splits(long long N, long long M) {
    if (N <= kSmallN) return 1;
    long long by_m = (kWantBlocks + M - 1) / M, by_n = (N + kMinPoints - 1) / kMinPoints;
    long long s = by_m < by_n ? by_m : by_n;
    return (int)(s < 1 ? 1 : (s > kMaxSplit ? kMaxSplit : s));
}

}   // namespace

extern "C" int32_t moda_near_far_splits(int64_t N, int64_t M) {
    if (N < 1 || M < 1) return 0;
    return auto_splits(N, M);
}

extern "C" int moda_frames_scatter(const float* rtk, const float* kaug, const float* rt_raw, const int64_t* frameid, int64_t bs,
                                   float* tab_rtk, float* tab_rt_raw, float* tab_idk, int64_t M, int32_t* status, void* stream) {
    if (bs < 0 || bs > MODA_FRAMES_MAX_BATCH || M < 1 || M > 0x7fffffffLL / 16) return MODA_ESHAPE;
    if (bs == 0) return 0;
    if (!rtk || !kaug || !rt_raw || !frameid || !tab_rtk || !tab_rt_raw || !tab_idk || !status) return MODA_EINVAL;
    hipLaunchKernelGGL(frames_scatter_kernel, dim3(nblocks(bs, kSmallBlock)), dim3(kSmallBlock), 0, (hipStream_t)stream, rtk, kaug,
                       rt_raw, (const long long*)frameid, (int)bs, tab_rtk, tab_rt_raw, tab_idk, (long long)M, (int*)status);
    return (int)hipGetLastError();
}

extern "C" int moda_near_far(const float* pts, int64_t N, float* tab_rtk, const float* idk, float* near_far, int64_t M,
                             double tol_fac, const float* rtk_all, int32_t splits, float* ws, int32_t* status, void* stream) {
    if (N < 1 || M < 1 || N > 0x7fffffffLL / 3 || M > 0x7fffffffLL / 16) return MODA_ESHAPE;
    if (splits < 0 || splits > kMaxSplit || (N <= kSmallN && splits > 1)) return MODA_EINVAL;
    if (!pts || !tab_rtk || !idk || !near_far || !status) return MODA_EINVAL;
    const float fac = (float)(tol_fac - 1.0);
    hipStream_t st = (hipStream_t)stream;
    if (N <= kSmallN) {
        hipLaunchKernelGGL(near_far_small_kernel, dim3(nblocks(M, kSmallBlock)), dim3(kSmallBlock), 0, st, pts, (int)N, tab_rtk, idk,
                           near_far, (long long)M, fac, rtk_all, (int*)status);
        return (int)hipGetLastError();
    }
    if (splits == 0) splits = auto_splits(N, M);
    if ((long long)splits > N) splits = (int)N;
    if (splits > 1 && !ws) return MODA_EINVAL;
    const long long per = (N + splits - 1) / splits;
    splits = (int)((N + per - 1) / per);                    // no empty range
    hipLaunchKernelGGL(near_far_block_kernel, dim3((unsigned)M, (unsigned)splits), dim3(kBlock), 0, st, pts, (long long)N, per, tab_rtk,
                       idk, near_far, fac, rtk_all, ws, (int*)status);
    if (splits > 1)
        hipLaunchKernelGGL(near_far_finish_kernel, dim3(nblocks(M, kSmallBlock)), dim3(kSmallBlock), 0, st, (const float*)ws, splits, idk,
                           near_far, (long long)M, fac, (int*)status);
    return (int)hipGetLastError();
}
