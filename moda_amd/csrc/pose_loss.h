// The rigid-pose loss vocabulary of lossasm_kernels.hip (second-order root smoothness) and warmup_kernels.hip (rtk_loss, first-
// order root smoothness): pose rows in and gradient rows out, the rotation angle between two poses (geom_utils.py:1196-1205
// rot_angle) with torch's clamp and its gradient, the video of a frame, and the sums of a one-workgroup forward.  Both files
// switch floating-point contraction off AFTER their includes, so every function here that multiplies and adds does it itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lanes.h"

namespace {

// torch's clamp(-1 + eps, 1 - eps) on an fp32 tensor: the bounds are formed in double and rounded to fp32 once
constexpr float kCosLo = (float)(-1.0 + 1e-4), kCosHi = (float)(1.0 - 1e-4);

DEVINL void load_pose(const float* __restrict__ rtk, int stride, long long f, float R[9], float t[3]) {
    const float* p = rtk + f * stride;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float4 r = *reinterpret_cast<const float4*>(p + 4 * i);       // rows of 4 floats, 16-byte aligned (host-checked)
        R[3 * i] = r.x; R[3 * i + 1] = r.y; R[3 * i + 2] = r.z; t[i] = r.w;
    }
}

// (trace(X Y^T) - 1) / 2: the diagonal entries with their products k = 0, 1, 2 added in that order, then 00 + 11 + 22
DEVINL float cos_of(const float X[9], const float Y[9]) {
#pragma clang fp contract(off)
    float tr = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float c = (X[3 * i] * Y[3 * i] + X[3 * i + 1] * Y[3 * i + 1]) + X[3 * i + 2] * Y[3 * i + 2];
        tr = i == 0 ? c : tr + c;
    }
    return (tr - 1.f) / 2.f;
}

DEVINL float angle_of(float c) { return acosf(fminf(fmaxf(c, kCosLo), kCosHi)); }

// d acos(clamp(c)) / dc: torch passes the gradient AT the (inclusive) bounds, and nothing outside them
DEVINL float dangle_of(float c) {
#pragma clang fp contract(off)
    return (c >= kCosLo && c <= kCosHi) ? -1.f / sqrtf(1.f - c * c) : 0.f;
}

// the video [start, end) frame f lies in; false when f belongs to none
DEVINL bool video_of(const int* __restrict__ off, int V, int T, int f, int& start, int& end) {
    for (int v = 0; v < V; ++v) {
        if (f >= off[v] && f < off[v + 1]) { start = max(off[v], 0); end = min(off[v + 1], T); return true; }   // (never past the array)
    }
    return false;
}

// frame f's gradient rows dR | dt as float4 stores (the fourth row of a 4 x 4 pose gets zeros)
DEVINL void store_pose_grad(float* __restrict__ drtk, int stride, long long f, const float dR[9], const float dt[3]) {
    float* p = drtk + f * stride;
#pragma unroll
    for (int i = 0; i < 3; ++i) *reinterpret_cast<float4*>(p + 4 * i) = make_float4(dR[3 * i], dR[3 * i + 1], dR[3 * i + 2], dt[i]);
    if (stride == 16) *reinterpret_cast<float4*>(p + 12) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// both sums and the count of a one-workgroup forward, joined in a fixed tree: lanes by wave_add's xor butterfly (32..1), waves in
// index order through LDS; the results are valid in thread 0
template <int WAVES>
DEVINL void block_sums(double& a, double& t, int& c, double* sh_a, double* sh_t, int* sh_c) {
    a = wave_add(a);
    t = wave_add(t);
    c = wave_add(c);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh_a[wave] = a; sh_t[wave] = t; sh_c[wave] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = 0.0; t = 0.0; c = 0;
        for (int w = 0; w < WAVES; ++w) { a += sh_a[w]; t += sh_t[w]; c += sh_c[w]; }
    }
}

// what every pose entry point asks of a pose array: rows of 4 floats (3 x 4 or 4 x 4 per frame), 16-byte aligned, T frames
inline bool pose_args_ok(const float* rtk, int32_t rows, int64_t T) {
    return rtk && (rows == 3 || rows == 4) && T >= 1 && T < (1 << 24) && al16(rtk);
}

}   // namespace
