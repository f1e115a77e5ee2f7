// Novel-view frame rendering, the two ends around render_rays (reference scripts/visualize/nvs.py:41-55 construct_rays_nvs and
// :160-174, the thresholding and the numpy scatter into `ones` canvases): a silhouette mask becomes a ray list, and the per-ray
// results become images.
//
//   mask_compact  masks (B,S,S) -> the list of kept pixels (value > 0) in frame-major, row-major order, the order of the
//                 reference's xys[:, rndmask].  A frame is cut into tiles of MODA_NVS_SCAN_TILE pixels, one workgroup each; a
//                 wave takes 256 consecutive pixels of its tile as four ballots of 64.
//                   1. tile sums     per wave the popcounts of its ballots, the four wave counts summed through LDS;
//                   2. tile offsets  ONE workgroup walks the tile sums 256 at a time (block_scan: shuffle scan in a wave, the four wave
//                                    totals through LDS; a running carry) -> the exclusive offset of every tile, and from the
//                                    first tile of every frame the frame offsets;
//                   3. tile scans    every tile takes its ballots again; a pixel's slot is its tile's offset + the counts of
//                                    the waves and ballots before it + the popcount of the lower lanes.
//                 Integer arithmetic in a fixed structure: the list has the same bits on every run.  rank (B,S,S) is the list's
//                 inverse (-1 outside the mask).
//   nvs_rays      one thread per listed pixel: xys, rays_d, rays_o, near, far from the pixel's frame; a second launch copies the
//                 per-frame rows (rtk_vec = [R | T | Kinv], env_code, time_embedded, bone_rts) to per-ray rows, one thread per
//                 output float.  rays_d and rays_o are written in the operation order the compiler gives raycast_kernel
//                 (prep_kernels.hip), spelled out with fmaf below, so that they carry moda_raycast's bits.
//   nvs_assemble  one thread per canvas pixel reads its rank and GATHERS its ray's results (or writes 1): no fill launch, no
//                 scatter, every output written once by consecutive lanes.
// No float atomics; device memory is written only by plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTile = MODA_NVS_SCAN_TILE;
constexpr int kWaveSpan = kTile / kWaves;          // consecutive pixels of a tile that one wave owns
constexpr int kPasses = kWaveSpan / 64;            // ballots per wave
static_assert(kTile % (kWaves * 64) == 0, "a tile is a whole number of ballots per wave");

template <bool U8>
DEVINL bool kept(const void* __restrict__ masks, long long i) {
    if (U8) return ((const uint8_t*)masks)[i] > 0;
    return ((const float*)masks)[i] > 0.0f;         // false for NaN, -0.0 and negatives
}

// the ballots of this wave's span of tile t; returns their popcount
template <bool U8>
DEVINL int wave_ballots(const void* __restrict__ masks, int P, int tpf, int t, int wave, int lane, unsigned long long m[kPasses],
                        int& b, int& first) {
    b = t / tpf;
    first = (t - b * tpf) * kTile + wave * kWaveSpan;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
        const int p = first + j * 64 + lane;
        m[j] = __ballot(p < P && kept<U8>(masks, (long long)b * P + p));
        cnt += __popcll(m[j]);
    }
    return cnt;
}

template <bool U8>
__global__ __launch_bounds__(kBlock) void tile_sums_kernel(const void* __restrict__ masks, int P, int tpf, int* __restrict__ tile_sums) {
    __shared__ int s_wave[kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long m[kPasses];
    int b, first;
    const int cnt = wave_ballots<U8>(masks, P, tpf, (int)blockIdx.x, wave, lane, m, b, first);
    if (lane == 0) s_wave[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += s_wave[w];
        tile_sums[blockIdx.x] = s;
    }
}

// one workgroup: exclusive scan of the T tile sums, and offsets[b] = the offset of frame b's first tile, offsets[B] = the total
__global__ __launch_bounds__(kBlock) void tile_offsets_kernel(const int* __restrict__ tile_sums, int T, int tpf, int B,
                                                              int* __restrict__ tile_off, int* __restrict__ offsets) {
    __shared__ int s_wave[kWaves];
    int carry = 0;
    for (int base = 0; base < T; base += kBlock) {
        const int i = base + (int)threadIdx.x;
        const int v = i < T ? tile_sums[i] : 0;
        const BlockScan<int> r = block_scan<int, kWaves>(v, s_wave);
        if (i < T) {
            const int excl = carry + r.before + r.incl_wave - v;
            tile_off[i] = excl;
            if (i % tpf == 0) offsets[i / tpf] = excl;
        }
        carry += r.total;
    }
    if (threadIdx.x == 0) offsets[B] = carry;
}

template <bool U8>
__global__ __launch_bounds__(kBlock) void tile_scan_kernel(const void* __restrict__ masks, int P, int tpf, const int* __restrict__ tile_off,
                                                           int cap, int* __restrict__ pix, int* __restrict__ frame,
                                                           int* __restrict__ rank) {
    __shared__ int s_wave[kWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long m[kPasses];
    int b, first;
    const int cnt = wave_ballots<U8>(masks, P, tpf, (int)blockIdx.x, wave, lane, m, b, first);
    if (lane == 0) s_wave[wave] = cnt;
    __syncthreads();
    int slot = tile_off[blockIdx.x];
#pragma unroll
    for (int w = 0; w < kWaves; ++w)
        if (w < wave) slot += s_wave[w];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < kPasses; ++j) {
        const int p = first + j * 64 + lane;
        const bool k = (m[j] >> lane) & 1ull;
        const int r = slot + __popcll(m[j] & below);      // < the total count: every kept pixel before this one has a lower slot
        if (k && r >= 0 && r < cap) {                     // (cap = B S S, the lists' size: holds unless the masks changed under the call)
            pix[r] = p;
            frame[r] = b;
        }
        if (p < P) rank[(long long)b * P + p] = k ? r : -1;
        slot += __popcll(m[j]);
    }
}

// ---- rays -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void nvs_rays_kernel(const int* __restrict__ pix, const int* __restrict__ frame, int n, int S, int B,
                                                          const float* __restrict__ Rm, const float* __restrict__ Tm,
                                                          const float* __restrict__ Kinv, const float* __restrict__ near_far,
                                                          float* __restrict__ xys, float* __restrict__ rays_d, float* __restrict__ rays_o,
                                                          float* __restrict__ near, float* __restrict__ far) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int f = frame[i], p = pix[i];
    const long long o2 = (long long)i * 2, o3 = (long long)i * 3;
    if (f < 0 || f >= B || p < 0 || p >= S * S) {          // not a list of moda_mask_compact: nothing is read through it
        const float nan = __uint_as_float(0x7fc00000u);
        xys[o2] = xys[o2 + 1] = near[i] = far[i] = nan;
        for (int c = 0; c < 3; ++c) rays_d[o3 + c] = rays_o[o3 + c] = nan;
        return;
    }
    const int yi = p / S;
    const float x = (float)(p - yi * S), y = (float)yi;
    float R[9], K[9], T[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) { R[k] = Rm[(long long)f * 9 + k]; K[k] = Kinv[(long long)f * 9 + k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) T[k] = Tm[(long long)f * 3 + k];
    // v = Kinv [x, y, 1], rays_d = v^T R, rays_o = -T^T R with raycast_kernel's roundings: one rounded product, then fused steps
    const float v0 = fmaf(K[1], y, K[0] * x) + K[2];
    const float v1 = fmaf(K[3], x, K[4] * y) + K[5];
    const float v2 = fmaf(K[6], x, K[7] * y) + K[8];
    xys[o2] = x;
    xys[o2 + 1] = y;
    rays_d[o3 + 0] = fmaf(v2, R[6], fmaf(v1, R[3], v0 * R[0]));
    rays_d[o3 + 1] = fmaf(v2, R[7], fmaf(v0, R[1], v1 * R[4]));
    rays_d[o3 + 2] = fmaf(v2, R[8], fmaf(v0, R[2], v1 * R[5]));
#pragma unroll
    for (int c = 0; c < 3; ++c) rays_o[o3 + c] = -fmaf(T[2], R[6 + c], fmaf(T[0], R[c], T[1] * R[3 + c]));
    near[i] = near_far[(long long)f * 2];
    far[i] = near_far[(long long)f * 2 + 1];
}

struct RowTable {
    const float* src;      // (B, C) rows; table 0 (rtk_vec) is read from Rmat, Tmat, Kinv instead
    float* dst;            // (n, C)
    int C;
};
struct RowArgs {
    RowTable t[4];
    const float *Rm, *Tm, *Kinv;
    const int* frame;
    int n, B;
};

// grid (x: output floats of the widest table, y: table); dst[i, c] = rows[frame[i], c]
__global__ __launch_bounds__(kBlock) void nvs_rows_kernel(RowArgs a) {
    const RowTable t = a.t[blockIdx.y];
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t.dst == nullptr || e >= (long long)a.n * t.C) return;
    const int i = (int)(e / t.C), c = (int)(e - (long long)i * t.C);
    const long long f = a.frame[i];
    float v = __uint_as_float(0x7fc00000u);
    if (f >= 0 && f < a.B) {
        if (blockIdx.y == 0) v = c < 9 ? a.Rm[f * 9 + c] : (c < 12 ? a.Tm[f * 3 + (c - 9)] : a.Kinv[f * 9 + (c - 12)]);
        else v = t.src[f * t.C + c];
    }
    t.dst[e] = v;
}

// ---- assembly ---------------------------------------------------------------------------------------------------------------
DEVINL uint8_t to_u8(float v) {                     // clip(rint(v * 255), 0, 255), round half to even, NaN -> 0
    const float t = v * 255.0f;
    if (!(t == t)) return 0;
    const float r = rintf(t);
    return (uint8_t)(r <= 0.0f ? 0.0f : (r >= 255.0f ? 255.0f : r));
}

__global__ __launch_bounds__(kBlock) void nvs_assemble_kernel(const int* __restrict__ rank, int N, int n, const float* __restrict__ rgb_in,
                                                              const float* __restrict__ depth_in, const float* __restrict__ sil_in,
                                                              const float* __restrict__ vis_in, float* __restrict__ rgb,
                                                              float* __restrict__ depth, float* __restrict__ sil, float* __restrict__ vis,
                                                              uint8_t* __restrict__ rgb8, uint8_t* __restrict__ sil8,
                                                              uint8_t* __restrict__ vis8) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= N) return;
    const int r = rank[e];
    float c[3] = {1.0f, 1.0f, 1.0f}, d = 1.0f, s = 1.0f, v = 1.0f;
    if (r >= 0 && r < n) {
        s = sil_in[r];
        const bool low = s < 0.5f;                 // false for NaN: the pixel keeps its NaN and its colour
        if (low) s = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = low ? 1.0f : rgb_in[(long long)r * 3 + k];
        d = depth_in[r];
        v = vis_in[r];
    }
    const long long e3 = (long long)e * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[e3 + k] = c[k];
    depth[e] = d;
    sil[e] = s;
    vis[e] = v;
    if (rgb8) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb8[e3 + k] = to_u8(c[k]);
        sil8[e] = to_u8(s);
        vis8[e] = to_u8(v);
    }
}

template <bool U8>
int compact(const void* masks, int B, int P, int tpf, int T, int* tile_sums, int* tile_off, int* offsets, int* pix, int* frame,
            int* rank, hipStream_t st) {
    hipLaunchKernelGGL(tile_sums_kernel<U8>, dim3((unsigned)T), dim3(kBlock), 0, st, masks, P, tpf, tile_sums);
    hipLaunchKernelGGL(tile_offsets_kernel, dim3(1), dim3(kBlock), 0, st, (const int*)tile_sums, T, tpf, B, tile_off, offsets);
    hipLaunchKernelGGL(tile_scan_kernel<U8>, dim3((unsigned)T), dim3(kBlock), 0, st, masks, P, tpf, (const int*)tile_off, B * P, pix, frame, rank);
    return (int)hipGetLastError();
}

}   // namespace

extern "C" int64_t moda_mask_compact_tiles(int64_t B, int64_t S) {
    if (B < 1 || S < 1 || S > 46340 || B > 0x7fffffffLL / (S * S)) return -1;
    const int64_t tiles = B * ((S * S + kTile - 1) / kTile);
    return tiles < MODA_NVS_MAX_TILES ? tiles : -1;
}

extern "C" int moda_mask_compact(const void* masks, int32_t is_u8, int64_t B, int64_t S, int32_t* tile_ws, int32_t* offsets,
                                 int32_t* pix, int32_t* frame, int32_t* rank, void* stream) {
    const int64_t T = moda_mask_compact_tiles(B, S);
    if (T < 0) return MODA_ESHAPE;
    if (!masks || !tile_ws || !offsets || !pix || !frame || !rank) return MODA_EINVAL;
    const int P = (int)(S * S), tpf = (P + kTile - 1) / kTile;
    int* sums = (int*)tile_ws;
    int* off = sums + T;
    return is_u8 ? compact<true>(masks, (int)B, P, tpf, (int)T, sums, off, (int*)offsets, (int*)pix, (int*)frame, (int*)rank, (hipStream_t)stream)
                 : compact<false>(masks, (int)B, P, tpf, (int)T, sums, off, (int*)offsets, (int*)pix, (int*)frame, (int*)rank, (hipStream_t)stream);
}

extern "C" int moda_nvs_rays(const int32_t* pix, const int32_t* frame, int64_t n, int64_t S, int64_t B, const float* Rmat, const float* Tmat,
                             const float* Kinv, const float* near_far, float* xys, float* rays_d, float* rays_o, float* near, float* far,
                             float* rtk_vec, const float* env_rows, int64_t env_c, float* env_out, const float* time_rows, int64_t time_c,
                             float* time_out, const float* bone_rows, int64_t bone_c, float* bone_out, void* stream) {
    if (n == 0) return 0;                                   // an empty list launches nothing
    if (n < 0 || n > 0x7fffffffLL || B < 1 || S < 1 || S > 46340 || B > 0x7fffffffLL / (S * S)) return MODA_ESHAPE;
    if (env_c < 0 || time_c < 0 || bone_c < 0 || env_c > 65536 || time_c > 65536 || bone_c > 65536) return MODA_ESHAPE;
    if (!pix || !frame || !Rmat || !Tmat || !Kinv || !near_far || !xys || !rays_d || !rays_o || !near || !far) return MODA_EINVAL;
    if ((env_out && (!env_rows || env_c < 1)) || (time_out && (!time_rows || time_c < 1)) || (bone_out && (!bone_rows || bone_c < 1)))
        return MODA_EINVAL;
    hipLaunchKernelGGL(nvs_rays_kernel, dim3(nblocks(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, (const int*)pix, (const int*)frame,
                       (int)n, (int)S, (int)B, Rmat, Tmat, Kinv, near_far, xys, rays_d, rays_o, near, far);
    RowArgs a;
    a.t[0] = {nullptr, rtk_vec, 21};
    a.t[1] = {env_rows, env_out, (int)env_c};
    a.t[2] = {time_rows, time_out, (int)time_c};
    a.t[3] = {bone_rows, bone_out, (int)bone_c};
    a.Rm = Rmat; a.Tm = Tmat; a.Kinv = Kinv; a.frame = (const int*)frame; a.n = (int)n; a.B = (int)B;
    int widest = 0;
    for (int k = 0; k < 4; ++k)
        if (a.t[k].dst && a.t[k].C > widest) widest = a.t[k].C;
    if (widest > 0) {
        const long long blocks = (n * widest + kBlock - 1) / kBlock;
        if (blocks >= MODA_NVS_MAX_TILES) return MODA_ESHAPE;          // 2^32 work-items a grid dimension
        hipLaunchKernelGGL(nvs_rows_kernel, dim3((unsigned)blocks, 4), dim3(kBlock), 0, (hipStream_t)stream, a);
    }
    return (int)hipGetLastError();
}

extern "C" int moda_nvs_assemble(const int32_t* rank, int64_t B, int64_t S, int64_t n, const float* rgb_in, const float* depth_in,
                                 const float* sil_in, const float* vis_in, float* rgb, float* depth, float* sil, float* vis,
                                 uint8_t* rgb8, uint8_t* sil8, uint8_t* vis8, void* stream) {
    if (B < 1 || S < 1 || S > 46340 || B > 0x7fffffffLL / (S * S) || n < 0 || n > B * S * S) return MODA_ESHAPE;
    if (!rank || !rgb || !depth || !sil || !vis || (n > 0 && (!rgb_in || !depth_in || !sil_in || !vis_in))) return MODA_EINVAL;
    if ((rgb8 != nullptr) != (sil8 != nullptr) || (rgb8 != nullptr) != (vis8 != nullptr)) return MODA_EINVAL;
    const long long N = B * S * S;
    hipLaunchKernelGGL(nvs_assemble_kernel, dim3(nblocks(N, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, (const int*)rank, (int)N, (int)n,
                       rgb_in, depth_in, sil_in, vis_in, rgb, depth, sil, vis, rgb8, sil8, vis8);
    return (int)hipGetLastError();
}
