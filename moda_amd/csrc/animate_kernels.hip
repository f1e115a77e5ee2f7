// Mesh sequence export: the rest mesh warped to every frame at once, and what the reference's eval() adds around it
// (nnutils/train_utils.py:522-593, utils/io.py:51-78 save_bones, :559-582 get_vertex_colors).
//
//   dqs_frames       out (F,V,3) = dqs_blend_skinning_chunk (geom_utils.py:457-493) of V points with FRAME-INDEPENDENT weights
//                    skin (V,B) under F sets of B dual quaternions.  One lane owns one vertex: its B weights and its point are
//                    loaded once into registers.  A workgroup walks the frames in tiles of MODA_ANIM_FRAME_TILE whose B x 8
//                    dual quaternions sit in LDS and are read through wave-uniform 16-byte loads (one address per wave: a
//                    broadcast, no bank conflict).  Per frame: bl = sum_b w_b dq_b in increasing b (fma), dq_normalize, the
//                    point transform (dqs_apply, moda_dev.h) -- what frame a tile holds, and where in it, changes no operand and
//                    no operation, so a frame's row has the same bits for every split of the frames over tiles and workgroups.
//                    The three coordinates of a wave's 64 vertices pass through a wave-private LDS row and leave as 192
//                    CONSECUTIVE floats (three full 256-byte stores), not as 64 stores at a 12-byte pitch.  No atomics.
//   color_dirs       the `dir_src` rows of get_vertex_colors for a chunk of frames, one thread per output float:
//                    [Embedding(normalize(vertex - camera centre)) | env_code row of the frame].
//   bone_ellipsoids  save_bones as one instancing launch: centre + R(q / |q|) (template / exp(scale)) per bone and template vertex.
//   skin_colors      (palette[None] * skin[..., None]).sum(1), in increasing bone order.
// Device memory is written only by plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "moda_dev.h"

namespace {

constexpr int kBlock = MODA_ANIM_BLOCK;
constexpr int kTile = MODA_ANIM_FRAME_TILE;
constexpr int kWaves = kBlock / 64;
constexpr int kStage = kBlock * 3;                  // floats of one staging buffer: 192 per wave
static_assert(kBlock % 64 == 0 && MODA_ANIM_MAX_BONES == 64, "whole waves; the instantiations below are 16, 32, 48 and 64 bones");

// LDS: [kTile x NB x 2] float4 (the tile's dual quaternions, bones B .. NB - 1 of a frame zero) | [2 x kStage] floats (output
// staging, two buffers so that one barrier a frame orders a wave's writes before its reads; a wave only ever touches its own
// 192 floats of a buffer).  NB = B rounded up to 16: the bone loop is unrolled without a branch (the weights need static
// register indices), and a padding bone adds fma(0, 0, bl) = bl, which changes no bit.
template <int NB>
__global__ __launch_bounds__(kBlock, 4) void dqs_frames_kernel(const float* __restrict__ dq, const float* __restrict__ skin,
                                                           const float* __restrict__ pts, int F, long long V, int B, int ntiles,
                                                           float* __restrict__ out) {
    extern __shared__ float4 lds4[];
    float* stage = (float*)(lds4 + kTile * NB * 2);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long long v0 = (long long)blockIdx.x * kBlock;
    const long long v = v0 + tid;
    const bool have = v < V;
    float w[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) w[b] = (have && b < B) ? skin[v * B + b] : 0.f;
    const float px = have ? pts[v * 3 + 0] : 0.f, py = have ? pts[v * 3 + 1] : 0.f, pz = have ? pts[v * 3 + 2] : 0.f;
    const long long wv0 = v0 + wave * 64;                                        // first vertex of this wave
    const long long left = (V - wv0) * 3;                                         // floats of this wave's row that exist
    const int nrow = left >= 192 ? 192 : (left > 0 ? (int)left : 0);
    for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
        const int f0 = t * kTile;
        const int nf = F - f0 < kTile ? F - f0 : kTile;
        __syncthreads();                                                          // the tile before has been read by every wave
        const float4* __restrict__ src = (const float4*)(dq + (long long)f0 * B * 8);
        for (int i = tid; i < nf * NB * 2; i += kBlock) {
            const int f = i / (NB * 2), r = i - f * (NB * 2);
            lds4[i] = r < B * 2 ? src[f * B * 2 + r] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
        for (int j = 0; j < nf; ++j) {
            const float4* q4 = lds4 + j * NB * 2;
            float bl[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const float4 r = q4[2 * b], d = q4[2 * b + 1];                    // one address per wave
                bl[0] = fmaf(w[b], r.x, bl[0]); bl[1] = fmaf(w[b], r.y, bl[1]);       // geom_utils.py:470
                bl[2] = fmaf(w[b], r.z, bl[2]); bl[3] = fmaf(w[b], r.w, bl[3]);
                bl[4] = fmaf(w[b], d.x, bl[4]); bl[5] = fmaf(w[b], d.y, bl[5]);
                bl[6] = fmaf(w[b], d.z, bl[6]); bl[7] = fmaf(w[b], d.w, bl[7]);
            }
            float ox, oy, oz;
            dqs_apply(bl, px, py, pz, &ox, &oy, &oz);                             // :471, :482-491
            float* st = stage + (j & 1) * kStage + wave * 192;
            st[lane * 3 + 0] = ox;
            st[lane * 3 + 1] = oy;
            st[lane * 3 + 2] = oz;
            __syncthreads();
            float* __restrict__ orow = out + ((long long)(f0 + j) * V + wv0) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int e = lane + 64 * k;
                if (e < nrow) orow[e] = st[e];
            }
        }
    }
}

struct Window { float w[16]; };

__global__ void color_dirs_kernel(const float* __restrict__ verts, const float* __restrict__ cam, const float* __restrict__ env,
                                  long long n, long long V, int n_freq, Window win, int Ce, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int Cd = 3 * (1 + 2 * n_freq), Wd = Cd + Ce;
    const long long r = i / Wd;
    const int c = (int)(i - r * Wd);
    const long long f = r / V;
    if (c >= Cd) {
        out[i] = env[f * Ce + (c - Cd)];                                          // io.py:564-565
        return;
    }
    const int grp = c / 3, ch = c - grp * 3;
    float v;
    if (cam) {                                                                    // train_utils.py:540-543, io.py:575
        const float dx = verts[r * 3 + 0] - cam[f * 3 + 0], dy = verts[r * 3 + 1] - cam[f * 3 + 1], dz = verts[r * 3 + 2] - cam[f * 3 + 2];
        const float nrm = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);      // F.normalize: x / max(|x|, eps)
        v = (ch == 0 ? dx : (ch == 1 ? dy : dz)) / nrm;
    } else {
        v = ch == 2 ? -1.f : 0.f;                                                 // io.py:570-573
    }
    if (grp > 0) {                                                                // nerf.py:35-75, as embed_kernel
        const int k = (grp - 1) >> 1;
        float sn, cs;
        sincosf(ldexpf(v, k), &sn, &cs);
        v = win.w[k] * (((grp - 1) & 1) ? cs : sn);
    }
    out[i] = v;
}

__global__ void bone_ellipsoids_kernel(const float* __restrict__ bones, long long n, const float* __restrict__ tmpl, int Nv,
                                       float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long nb = i / Nv;
    const int t = (int)(i - nb * Nv);
    const float* b = bones + nb * 10;
    const float nrm = sqrtf(b[3] * b[3] + b[4] * b[4] + b[5] * b[5] + b[6] * b[6]);       // io.py:60-61
    Quat q = {b[3] / nrm, b[4] / nrm, b[5] / nrm, b[6] / nrm};
    float R[9];
    quat_to_mat(q, R);
    const float sx = tmpl[t * 3 + 0] / expf(b[7]), sy = tmpl[t * 3 + 1] / expf(b[8]), sz = tmpl[t * 3 + 2] / expf(b[9]);   // :65-68
    out[i * 3 + 0] = b[0] + (R[0] * sx + R[1] * sy + R[2] * sz);                  // :69-70: verts @ R^T + centre
    out[i * 3 + 1] = b[1] + (R[3] * sx + R[4] * sy + R[5] * sz);
    out[i * 3 + 2] = b[2] + (R[6] * sx + R[7] * sy + R[8] * sz);
}

__global__ void skin_colors_kernel(const float* __restrict__ skin, const float* __restrict__ pal, long long V, int B,
                                   float* __restrict__ out) {
    const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    float r = 0.f, g = 0.f, bb = 0.f;
    for (int b = 0; b < B; ++b) {                                                 // train_utils.py:587
        const float w = skin[v * B + b];
        r = fmaf(pal[b * 3 + 0], w, r);
        g = fmaf(pal[b * 3 + 1], w, g);
        bb = fmaf(pal[b * 3 + 2], w, bb);
    }
    out[v * 3 + 0] = r;
    out[v * 3 + 1] = g;
    out[v * 3 + 2] = bb;
}

}   // namespace

extern "C" int moda_dqs_frames(const float* dq, const float* skin, const float* pts, int64_t F, int64_t V, int32_t B,
                               int32_t frame_splits, float* out, void* stream) {
    if (F < 1 || V < 1 || B < 1 || B > MODA_ANIM_MAX_BONES || F > 0x7fffffffLL || V > 0x7fffffffLL || frame_splits < 0)
        return MODA_ESHAPE;
    if (V > 0x7fffffffffffffffLL / (3 * F) / 4 || V * B > 0x7fffffffffffLL) return MODA_ESHAPE;
    if (!dq || !skin || !pts || !out || ((uintptr_t)dq & 15)) return MODA_EINVAL;
    const int ntiles = (int)((F + kTile - 1) / kTile);
    const unsigned gx = nblocks(V, kBlock);
    // enough workgroups to fill the chip when the mesh is small; every split gives the same bits
    long long gy = frame_splits > 0 ? frame_splits : (2048 + gx - 1) / gx;
    if (gy > ntiles) gy = ntiles;
    if (gy > 65535) gy = 65535;
    const int NB = (B + 15) / 16 * 16;
    const size_t lds = (size_t)kTile * NB * 2 * sizeof(float4) + 2 * kStage * sizeof(float);
#define MODA_ANIM_LAUNCH(N)                                                                                                       \
    hipLaunchKernelGGL(dqs_frames_kernel<N>, dim3(gx, (unsigned)gy), dim3(kBlock), lds, (hipStream_t)stream, dq, skin, pts, (int)F, \
                       (long long)V, (int)B, ntiles, out)
    if (NB == 16) MODA_ANIM_LAUNCH(16);
    else if (NB == 32) MODA_ANIM_LAUNCH(32);
    else if (NB == 48) MODA_ANIM_LAUNCH(48);
    else MODA_ANIM_LAUNCH(64);
#undef MODA_ANIM_LAUNCH
    return (int)hipGetLastError();
}

extern "C" int moda_color_dirs(const float* verts, const float* cam, const float* env, int64_t Fc, int64_t V, int32_t n_freq,
                               const float* window, int32_t Ce, float* out, void* stream) {
    if (Fc < 1 || V < 1 || n_freq < 0 || n_freq > 16 || Ce < 0 || Ce > 65536) return MODA_ESHAPE;
    const long long Wd = 3 * (1 + 2 * n_freq) + Ce;
    if (Fc > 0x7fffffffLL || V > 0x7fffffffLL || Fc * V > 0x7fffffffffffLL / Wd) return MODA_ESHAPE;
    const long long n = Fc * V * Wd;
    if ((n + kBlock - 1) / kBlock > 0x7fffffffLL) return MODA_ESHAPE;
    if (!out || (Ce > 0 && !env) || (n_freq > 0 && !window) || ((verts != nullptr) != (cam != nullptr))) return MODA_EINVAL;
    Window w;
    for (int k = 0; k < 16; ++k) w.w[k] = k < n_freq ? window[k] : 0.f;
    hipLaunchKernelGGL(color_dirs_kernel, dim3(nblocks(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, verts, cam, env, n, (long long)V,
                       (int)n_freq, w, (int)Ce, out);
    return (int)hipGetLastError();
}

extern "C" int moda_bone_ellipsoids(const float* bones, int64_t n_bones, const float* tmpl, int32_t Nv, float* out, void* stream) {
    if (n_bones < 1 || Nv < 1 || n_bones > 0x7fffffffLL || n_bones * Nv > 0x7fffffffLL * kBlock / 4) return MODA_ESHAPE;
    if (!bones || !tmpl || !out) return MODA_EINVAL;
    const long long n = n_bones * Nv;
    hipLaunchKernelGGL(bone_ellipsoids_kernel, dim3(nblocks(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, bones, n, tmpl, (int)Nv, out);
    return (int)hipGetLastError();
}

extern "C" int moda_skin_colors(const float* skin, const float* palette, int64_t V, int32_t B, float* out, void* stream) {
    if (V < 1 || B < 1 || V > 0x7fffffffLL || B > 65536) return MODA_ESHAPE;
    if (!skin || !palette || !out) return MODA_EINVAL;
    hipLaunchKernelGGL(skin_colors_kernel, dim3(nblocks(V, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, skin, palette, (long long)V, (int)B,
                       out);
    return (int)hipGetLastError();
}
