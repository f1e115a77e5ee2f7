// Mesh rasteriser, forward only: the reference's soft_rasterize kernel (third_party/softras/soft_renderer/cuda/
// soft_rasterize_cuda_kernel.cu:246-483) in the one configuration MoDA uses (nnutils/moda.py:469-471: sigma_val = 1e-12, hard
// rgb aggregation, prod alpha, vertex textures, fill_back = double_side, near 1, far 100, no anti-aliasing), restated as
//
//   face_setup   one thread per (view, face): the inverse edge matrix with the determinant clamped at +-1e-10 (:274-286), the
//                corner depths, and the box of pixels whose centres can lie in the face (its bounding box in pixel units, one
//                pixel wider on every side: the fp32 inside test can only differ from the exact one within rounding of an edge).
//                A face is EMPTY (never tested) when a vertex index is outside [0, V), when the box misses the image, or when
//                the float64 determinant is exactly 0 (the reference's clamp makes its barycentrics meaningless; it draws nothing).
//   raster_tile  one 256-lane workgroup per (view, 16 x 16 pixel tile), one pixel per lane.  The workgroup walks the face boxes of
//                its view 256 at a time, one per lane; the faces whose box meets the tile are compacted into LDS IN ASCENDING FACE
//                ORDER (wave ballots + a prefix over the four waves), and whenever 256 or more are waiting their 96-byte records
//                are staged into LDS and every lane tests its pixel against each of them, reading a record at a wave-uniform
//                address (a broadcast: no bank conflict).  Each lane keeps its best (zp, face, w_clip) in registers; a strict <
//                in ascending face order keeps the lowest face index among equal depths (:429).  One store per pixel at the end.
//                The per-tile lists therefore never exist in global memory: nothing data dependent is sized, scanned or read
//                back, and no atomic touches the image.  The price is that every tile, also one that no face touches, reads
//                every face box of its view (16 bytes per face from L2): S^2 / 256 * F box tests per view, 1/256 of the
//                reference's per-pixel loop over all faces.
//                binned = 0 sends every non-empty face to every tile (the unbinned route the tests compare bit for bit).
//   raster_interp one thread per (view, pixel): out[c] = w0 a0[c] + w1 a1[c] + w2 a2[c] (:190-191) for any number of channels,
//                one fixed product + two FMAs per channel, so a channel's bits do not depend on how many channels ride along.
//
// Arithmetic: the edge equations and the barycentrics w_k = A_k x + B_k y + C_k are float64, from the fp32 vertices and float64
// pixel centres.  The three terms are of size |x| / (height of the face) and cancel; in fp32 (the reference's scalar_t) that
// costs 1e-3 and more in w on the foreshortened faces at the limb of a sphere (height 1e-5 NDC), measured against the float64
// oracle.  Everything after the inside test (clip, depth, the outputs) is fp32 as in the reference.
// NOT YET TIMED: neither the binning inside the tile kernel (against a count / scan / fill pass) nor the float64 w has a
// measurement behind it; tools/raster_bench.py is the tool, and its first run decides whether these choices stay.
// alpha is the hard cover mask: with sigma_val = 1e-12 the reference's prod aggregate is 1 where a face covers the pixel centre
// and 0 elsewhere, except within about 3e-6 NDC of an edge (:352, :399-403, :415-416); it is taken BEFORE the near / far test
// (:408-424), so a face outside the depth range sets alpha without colouring the pixel.
// Device memory is written only by plain vector stores.  Indices are int32; element offsets are formed in 64 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kTile = MODA_RASTER_TILE;    // 16 x 16 pixels = one lane per pixel
constexpr int kList = 2 * kBlock;          // faces waiting in LDS: fewer than kBlock before a step adds at most kBlock

// pixel-centre coordinate of column / flipped row index i (:343-346)
DEVINL double pixel_centre(int i, int S) { return (2.0 * (double)i + 1.0 - (double)S) / (double)S; }

// rec (B*F, 12) double = (A_k, B_k, C_k, z_k) per corner k: w_k = A_k x + B_k y + C_k.  box (B*F) int4 = (col0, row0, col1, row1)
// inclusive, image rows (row 0 = the largest y); col0 > col1 marks an empty face.
__global__ __launch_bounds__(kBlock) void face_setup_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                            int64_t face_stride, int64_t total, int V, int F, int S,
                                                            double* __restrict__ rec, int4* __restrict__ box) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / F;
    const int f = (int)(i - b * F);
    const int* fv = faces + b * face_stride + (int64_t)f * 3;
    const int i0 = fv[0], i1 = fv[1], i2 = fv[2];
    int4 bx = make_int4(1, 1, 0, 0);
    double r[12] = {0., 0., 0., 1., 0., 0., 0., 1., 0., 0., 0., 1.};
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {         // never read through a bad index
        const float* vb = verts + b * (int64_t)V * 3;
        const float x0 = vb[(int64_t)i0 * 3], y0 = vb[(int64_t)i0 * 3 + 1], z0 = vb[(int64_t)i0 * 3 + 2];
        const float x1 = vb[(int64_t)i1 * 3], y1 = vb[(int64_t)i1 * 3 + 1], z1 = vb[(int64_t)i1 * 3 + 2];
        const float x2 = vb[(int64_t)i2 * 3], y2 = vb[(int64_t)i2 * 3 + 1], z2 = vb[(int64_t)i2 * 3 + 2];
        const double X0 = x0, Y0 = y0, X1 = x1, Y1 = y1, X2 = x2, Y2 = y2;
        double det = X2 * (Y0 - Y1) + X0 * (Y1 - Y2) + X1 * (Y2 - Y0);           // :278-281
        const bool flat = det == 0.0;
        det = det > 0.0 ? fmax(det, 1e-10) : fmin(det, -1e-10);                 // :282
        r[0] = (Y1 - Y2) / det, r[1] = (X2 - X1) / det, r[2] = (X1 * Y2 - X2 * Y1) / det, r[3] = z0;        // :274-277, :285
        r[4] = (Y2 - Y0) / det, r[5] = (X0 - X2) / det, r[6] = (X2 * Y0 - X0 * Y2) / det, r[7] = z1;
        r[8] = (Y0 - Y1) / det, r[9] = (X1 - X0) / det, r[10] = (X0 * Y1 - X1 * Y0) / det, r[11] = z2;
        // pixel index of a coordinate: centre(i) = (2 i + 1 - S) / S  <=>  i = ((x + 1) S - 1) / 2; clamped before the
        // conversion so that no value, however large, reaches an int out of range (fmaxf / fminf drop a NaN operand)
        const float lim = (float)S + 1.f;
        const float cx0 = fminf(fmaxf(((fminf(fminf(x0, x1), x2) + 1.f) * (float)S - 1.f) * 0.5f, -2.f), lim);
        const float cx1 = fminf(fmaxf(((fmaxf(fmaxf(x0, x1), x2) + 1.f) * (float)S - 1.f) * 0.5f, -2.f), lim);
        const float cy0 = fminf(fmaxf(((fminf(fminf(y0, y1), y2) + 1.f) * (float)S - 1.f) * 0.5f, -2.f), lim);
        const float cy1 = fminf(fmaxf(((fmaxf(fmaxf(y0, y1), y2) + 1.f) * (float)S - 1.f) * 0.5f, -2.f), lim);
        const int c0 = max((int)ceilf(cx0) - 1, 0), c1 = min((int)floorf(cx1) + 1, S - 1);
        const int yi0 = max((int)ceilf(cy0) - 1, 0), yi1 = min((int)floorf(cy1) + 1, S - 1);
        if (!flat && c0 <= c1 && yi0 <= yi1) bx = make_int4(c0, S - 1 - yi1, c1, S - 1 - yi0);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) rec[i * 12 + k] = r[k];
    box[i] = bx;
}

__global__ __launch_bounds__(kBlock) void raster_tile_kernel(const double* __restrict__ rec, const int4* __restrict__ box, int F,
                                                             int S, int tiles, float near, float far, int binned,
                                                             int* __restrict__ face_idx, float* __restrict__ bary,
                                                             float* __restrict__ zbuf, float* __restrict__ alpha) {
    __shared__ double s_rec[kList][12];                                         // 48 KB
    __shared__ int s_face[kList];
    __shared__ int s_wave[kBlock / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per_view = tiles * tiles;
    const int b = blockIdx.x / per_view, tile = blockIdx.x - b * per_view;
    const int ty = tile / tiles, tx = tile - ty * tiles;
    const int col = tx * kTile + (t & (kTile - 1)), row = ty * kTile + (t >> 4);
    const int tc0 = tx * kTile, tc1 = tc0 + kTile - 1, tr0 = ty * kTile, tr1 = tr0 + kTile - 1;
    const double xp = pixel_centre(col, S), yp = pixel_centre(S - 1 - row, S);  // lanes past the image compute and do not store
    const double* rec_b = rec + (int64_t)b * F * 12;
    const int4* box_b = box + (int64_t)b * F;

    float best = 10000000.f;                                                    // :367
    int best_f = -1;
    float bw0 = 0.f, bw1 = 0.f, bw2 = 0.f;
    bool covered = false;
    int n_list = 0;                                                             // the same value in every lane

    for (int f0 = 0; f0 < F; f0 += kBlock) {
        const int f = f0 + t;
        bool hit = false;
        if (f < F) {
            const int4 bx = box_b[f];
            hit = bx.x <= bx.z && (!binned || (bx.x <= tc1 && bx.z >= tc0 && bx.y <= tr1 && bx.w >= tr0));
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = n_list, total = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
            const int c = s_wave[w];
            if (w < wave) before += c;
            total += c;
        }
        if (hit) s_face[before + __popcll(m & ((1ull << lane) - 1ull))] = f;    // < n_list + total <= kList - 1
        n_list += total;
        const bool last = f0 + kBlock >= F;
        if (n_list >= kBlock || (last && n_list > 0)) {
            __syncthreads();                                                    // s_face is complete
            for (int j = t; j < n_list * 12; j += kBlock)                       // consecutive lanes, consecutive words
                s_rec[j / 12][j % 12] = rec_b[(int64_t)s_face[j / 12] * 12 + j % 12];
            __syncthreads();
            for (int j = 0; j < n_list; ++j) {
                const double* e = s_rec[j];
                const double d0 = __builtin_fma(e[0], xp, __builtin_fma(e[1], yp, e[2]));       // :26-28
                const double d1 = __builtin_fma(e[4], xp, __builtin_fma(e[5], yp, e[6]));
                const double d2 = __builtin_fma(e[8], xp, __builtin_fma(e[9], yp, e[10]));
                if (!(d0 <= 1.0 && d0 >= 0.0 && d1 <= 1.0 && d1 >= 0.0 && d2 <= 1.0 && d2 >= 0.0)) continue;   // :47-50
                const float w0 = (float)d0, w1 = (float)d1, w2 = (float)d2;
                const float z0 = (float)e[3], z1 = (float)e[7], z2 = (float)e[11];
                covered = true;                                                 // alpha, before the depth range (:408-417)
                const float sum = fmaxf(w0 + w1 + w2, 1e-5f);                   // :53-58 (inside: the clip to [0, 1] is a no-op)
                const float c0 = w0 / sum, c1 = w1 / sum, c2 = w2 / sum;
                const float zp = 1.f / (c0 / z0 + c1 / z1 + c2 / z2);     // :423
                if (zp < near || zp > far) continue;                            // :424
                if (zp < best) {                                                // :429: ascending faces, the first of equals stays
                    best = zp;
                    best_f = s_face[j];
                    bw0 = c0;
                    bw1 = c1;
                    bw2 = c2;
                }
            }
            n_list = 0;
        }
        __syncthreads();                                                        // s_wave, s_face and s_rec may be rewritten
    }
    if (col < S && row < S) {
        const int64_t o = ((int64_t)b * S + row) * S + col;
        face_idx[o] = best_f;
        bary[o * 3 + 0] = bw0;
        bary[o * 3 + 1] = bw1;
        bary[o * 3 + 2] = bw2;
        zbuf[o] = best_f >= 0 ? best : 0.f;
        alpha[o] = covered ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(kBlock) void raster_interp_kernel(const float* __restrict__ attrs, const int* __restrict__ faces,
                                                               int64_t face_stride, const int* __restrict__ face_idx,
                                                               const float* __restrict__ bary, const float* __restrict__ bg,
                                                               int64_t total, int V, int F, int C, int64_t SS,
                                                               float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / SS, p = i - b * SS;
    float* o = out + b * C * SS + p;
    const int f = face_idx[i];
    int i0 = -1, i1 = -1, i2 = -1;
    if (f >= 0 && f < F) {
        const int* fv = faces + b * face_stride + (int64_t)f * 3;
        i0 = fv[0], i1 = fv[1], i2 = fv[2];
    }
    if (!(i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V)) {       // nothing drawn here: the background
        for (int c = 0; c < C; ++c) o[(int64_t)c * SS] = bg ? bg[c] : 0.f;
        return;
    }
    const float w0 = bary[i * 3 + 0], w1 = bary[i * 3 + 1], w2 = bary[i * 3 + 2];
    const float* a = attrs + b * (int64_t)V * C;
    const float* a0 = a + (int64_t)i0 * C;
    const float* a1 = a + (int64_t)i1 * C;
    const float* a2 = a + (int64_t)i2 * C;
    for (int c = 0; c < C; ++c)
        o[(int64_t)c * SS] = __builtin_fmaf(w2, a2[c], __builtin_fmaf(w1, a1[c], w0 * a0[c]));  // :190-191
}

bool raster_shape_ok(int64_t B, int64_t V, int64_t F, int64_t S) {
    if (B < 1 || V < 1 || F < 1 || S < 1 || S > 32768 || V >= 2147483648LL) return false;
    return (double)B * (double)S * (double)S < 2147483648.0 && (double)B * (double)F < 2147483648.0;
}

}   // namespace

extern "C" int moda_raster_fwd(const float* verts, const int32_t* faces, int32_t faces_per_view, int64_t B, int64_t V, int64_t F,
                               int64_t S, float near, float far, int32_t binned, double* rec, int32_t* box, int32_t* face_idx,
                               float* bary, float* zbuf, float* alpha, void* stream) {
    if (!raster_shape_ok(B, V, F, S)) return MODA_ESHAPE;
    const int64_t tiles = (S + kTile - 1) / kTile;
    if ((double)B * (double)tiles * (double)tiles >= 2147483648.0) return MODA_ESHAPE;
    if (!verts || !faces || !rec || !box || !face_idx || !bary || !zbuf || !alpha) return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(face_setup_kernel, dim3(nblocks(B * F, kBlock)), dim3(kBlock), 0, st, verts, faces,
                       faces_per_view ? F * 3 : (int64_t)0, B * F, (int)V, (int)F, (int)S, rec, (int4*)box);
    hipLaunchKernelGGL(raster_tile_kernel, dim3((unsigned)(B * tiles * tiles)), dim3(kBlock), 0, st, (const double*)rec,
                       (const int4*)box, (int)F, (int)S, (int)tiles, near, far, binned ? 1 : 0, face_idx, bary, zbuf, alpha);
    return (int)hipGetLastError();
}

extern "C" int moda_raster_interp(const float* attrs, const int32_t* faces, int32_t faces_per_view, const int32_t* face_idx,
                                  const float* bary, const float* background, int64_t B, int64_t V, int64_t F, int64_t C,
                                  int64_t S, float* out, void* stream) {
    if (!raster_shape_ok(B, V, F, S) || C < 1 || C > 65536) return MODA_ESHAPE;
    if ((double)B * (double)S * (double)S * (double)C >= 9.0e18 || (double)B * (double)V * (double)C >= 9.0e18) return MODA_ESHAPE;
    if (!attrs || !faces || !face_idx || !bary || !out) return MODA_EINVAL;
    hipLaunchKernelGGL(raster_interp_kernel, dim3(nblocks(B * S * S, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, attrs, faces,
                       faces_per_view ? F * 3 : (int64_t)0, face_idx, bary, background, B * S * S, (int)V, (int)F, (int)C, S * S,
                       out);
    return (int)hipGetLastError();
}
