// Frame-pair preparation (reference dataloader/vidbase.py:142-246: compute_crop_params, the six cv2.remap calls of read_raw,
// flow_process with warp_flow; nnutils/moda.py:1362-1417 convert_batch_input's pair-major order and silhouette rule).
// fp32 data, float64 coordinates.
//
//   mask_bbox    per frame the box xmin, xmax, ymin, ymax of the pixels > 0.  Threads walk the frame coalesced (four pixels a
//                load when the frame's pixel count allows), keep their own min / max, a wave folds them with shuffles and its
//                first lane issues at most four integer atomicMin / atomicMax: order-independent, the same bits on every run.
//   crop_params  one thread per frame: centre and half-length by integer // 2, int(crop_factor * length) as a float64 product
//                truncated toward zero, alp = 2 length / img_size in float64.  An empty mask or a half-length of 0 is counted
//                in the status word and gives NaN rows, which every later kernel answers with zeros instead of reading through.
//   crop_remap   one thread per output pixel; the source coordinate x = col * alp0 + tx is one float64 multiply and one add
//                (never contracted), rounded to fp32 as the reference's .astype(np.float32), and every plane is sampled from
//                that one coordinate.  Output frames are written in convert_batch_input's order (all first frames, then all
//                second frames).
//   sampler      cv2.remap with float maps and the constant-zero border, restated: linear -- sx = rne(x * 32), cell sx >> 5,
//                fraction sx & 31, the four weights (1 - f/32, f/32) x (1 - g/32, g/32) (exact in fp32), summed left to right,
//                a tap outside the image contributes 0; nearest -- rne(x), 0 outside.  A coordinate that is NaN, infinite or
//                beyond 2^25 in magnitude is outside every image: the result is 0.
//   flow_process both directions of a pair in one launch, no intermediate image: the flow re-expressed in the other frame's crop
//                by the closed-form inverse of its affine, the forward-backward check recomputed at the four taps from the
//                cropped flow of the other frame, occ = exp(-25 * 2 |dis| / img_size) zeroed below 0.25, flows scaled to NDC.
// Device memory is written only by plain vector stores and HIP atomic functions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kBboxMaxBlocks = 1024;             // workgroups per frame of the box reduction

// ---- the sampler ------------------------------------------------------------------------------------------------------------
struct Taps {
    int x0, y0;              // the cell's top-left pixel
    float w00, w01, w10, w11;
    bool ok;                 // false: the coordinate is not a usable number, the sample is 0
};

DEVINL bool fixed5(float x, int& cell, int& frac) {
    const float s = x * 32.0f;
    if (!(fabsf(s) < 1073741824.0f)) return false;                         // NaN, inf, beyond 2^25: outside every image
    const int i = (int)rintf(s);                                           // round half to even
    cell = i >> 5;
    frac = i & 31;
    return true;
}

DEVINL Taps linear_taps(float x, float y) {
    Taps t;
    int fx = 0, fy = 0;
    t.x0 = t.y0 = 0;
    t.ok = fixed5(x, t.x0, fx) & fixed5(y, t.y0, fy);
    const float ax = (float)fx * 0.03125f, ay = (float)fy * 0.03125f;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    t.w00 = by * bx;
    t.w01 = by * ax;
    t.w10 = ay * bx;
    t.w11 = ay * ax;
    return t;
}

DEVINL bool nearest_px(float x, float y, int W, int H, int& xi, int& yi) {
    if (!(fabsf(x) < 1073741824.0f) || !(fabsf(y) < 1073741824.0f)) return false;
    xi = (int)rintf(x);
    yi = (int)rintf(y);
    return xi >= 0 && xi < W && yi >= 0 && yi < H;
}

// the four taps of a plane whose pixel (x, y) lies at base[(y * W + x) * stride]; a tap outside the image is 0
template <typename T>
DEVINL float blend(const T* __restrict__ base, int64_t stride, int W, int H, const Taps& t, float scale_div) {
    if (!t.ok) return 0.0f;
    const bool xa = t.x0 >= 0 && t.x0 < W, xb = t.x0 + 1 >= 0 && t.x0 + 1 < W;
    const bool ya = t.y0 >= 0 && t.y0 < H, yb = t.y0 + 1 >= 0 && t.y0 + 1 < H;
    const int64_t o = ((int64_t)t.y0 * W + t.x0) * stride;
    float v00 = xa && ya ? (float)base[o] : 0.0f;
    float v01 = xb && ya ? (float)base[o + stride] : 0.0f;
    float v10 = xa && yb ? (float)base[o + (int64_t)W * stride] : 0.0f;
    float v11 = xb && yb ? (float)base[o + (int64_t)W * stride + stride] : 0.0f;
    if (scale_div != 0.0f) {
        v00 = v00 / scale_div;
        v01 = v01 / scale_div;
        v10 = v10 / scale_div;
        v11 = v11 / scale_div;
    }
    return ((v00 * t.w00 + v01 * t.w01) + v10 * t.w10) + v11 * t.w11;
}

// ---- mask_bbox --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void bbox_init_kernel(int* __restrict__ box, int B, int h, int w) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    box[b * 4 + 0] = w;
    box[b * 4 + 1] = -1;
    box[b * 4 + 2] = h;
    box[b * 4 + 3] = -1;
}

struct Box {
    int x0, x1, y0, y1;
};

DEVINL void box_add(Box& bx, int p, int w) {
    const int y = p / w, x = p - y * w;
    bx.x0 = min(bx.x0, x);
    bx.x1 = max(bx.x1, x);
    bx.y0 = min(bx.y0, y);
    bx.y1 = max(bx.y1, y);
}

template <bool U8>
__global__ __launch_bounds__(kBlock) void bbox_kernel(const void* __restrict__ masks, int h, int w, int* __restrict__ box) {
    const int b = blockIdx.y;
    const int hw = h * w;
    Box bx = {w, -1, h, -1};
    const int step = gridDim.x * kBlock;
    if ((hw & 3) == 0) {                                                   // every frame starts on a 4-pixel boundary
        const int n4 = hw >> 2;
        for (int q = blockIdx.x * kBlock + threadIdx.x; q < n4; q += step) {
            if (U8) {
                const uint32_t v = ((const uint32_t*)masks)[(int64_t)b * n4 + q];
                if (v) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if ((v >> (8 * k)) & 0xFFu) box_add(bx, q * 4 + k, w);
                }
            } else {
                const float4 v = ((const float4*)masks)[(int64_t)b * n4 + q];
                if (v.x > 0.0f) box_add(bx, q * 4 + 0, w);
                if (v.y > 0.0f) box_add(bx, q * 4 + 1, w);
                if (v.z > 0.0f) box_add(bx, q * 4 + 2, w);
                if (v.w > 0.0f) box_add(bx, q * 4 + 3, w);
            }
        }
    } else {
        for (int p = blockIdx.x * kBlock + threadIdx.x; p < hw; p += step) {
            const bool on = U8 ? ((const uint8_t*)masks)[(int64_t)b * hw + p] > 0 : ((const float*)masks)[(int64_t)b * hw + p] > 0.0f;
            if (on) box_add(bx, p, w);
        }
    }
    const auto lower = [](int x, int y) { return min(x, y); };
    const auto upper = [](int x, int y) { return max(x, y); };
    bx.x0 = wave_all(bx.x0, lower);
    bx.x1 = wave_all(bx.x1, upper);
    bx.y0 = wave_all(bx.y0, lower);
    bx.y1 = wave_all(bx.y1, upper);
    if ((threadIdx.x & 63) == 0 && bx.x1 >= 0) {
        atomicMin(&box[b * 4 + 0], bx.x0);
        atomicMax(&box[b * 4 + 1], bx.x1);
        atomicMin(&box[b * 4 + 2], bx.y0);
        atomicMax(&box[b * 4 + 3], bx.y1);
    }
}

// ---- crop_params ------------------------------------------------------------------------------------------------------------
DEVINL int out_frame(int f, int bs) { return bs > 0 ? (f & 1) * bs + (f >> 1) : f; }     // (pair, k) -> k * bs + pair
DEVINL int src_frame(int o, int bs) { return bs > 0 ? (o % bs) * 2 + o / bs : o; }
DEVINL int partner(int o, int bs) { return o < bs ? o + bs : o - bs; }

__global__ __launch_bounds__(kBlock) void crop_params_kernel(const int* __restrict__ box, int B, int bs, int img_size, double factor,
                                                            float* __restrict__ kaug, double* __restrict__ aff,
                                                            int* __restrict__ status) {
    const int f = blockIdx.x * kBlock + threadIdx.x;
    if (f >= B) return;
    const int x0 = box[f * 4 + 0], x1 = box[f * 4 + 1], y0 = box[f * 4 + 2], y1 = box[f * 4 + 3];
    const int o = out_frame(f, bs);
    const bool empty = x1 < x0 || y1 < y0 || x0 < 0 || y0 < 0;
    int Lx = 0, Ly = 0, cx = 0, cy = 0;
    if (!empty) {
        cx = (x1 + x0) / 2;                                                // non-negative: / is //
        cy = (y1 + y0) / 2;
        Lx = (int)(factor * (double)((x1 - x0) / 2));                      // int(): toward zero
        Ly = (int)(factor * (double)((y1 - y0) / 2));
    }
    if (empty || Lx <= 0 || Ly <= 0) {
        if (status) atomicAdd(&status[empty ? 0 : 1], 1);
        const float qn = __int_as_float(0x7FC00000);
        const double dn = (double)qn;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            kaug[o * 4 + k] = qn;
            aff[o * 4 + k] = dn;
        }
        return;
    }
    const double a0 = (double)(2 * Lx) / (double)img_size, a1 = (double)(2 * Ly) / (double)img_size;
    const double tx = (double)(cx - Lx), ty = (double)(cy - Ly);
    aff[o * 4 + 0] = a0;
    aff[o * 4 + 1] = a1;
    aff[o * 4 + 2] = tx;
    aff[o * 4 + 3] = ty;
    kaug[o * 4 + 0] = (float)a0;
    kaug[o * 4 + 1] = (float)a1;
    kaug[o * 4 + 2] = (float)tx;
    kaug[o * 4 + 3] = (float)ty;
}

// ---- crop_remap -------------------------------------------------------------------------------------------------------------
struct CropArgs {
    const uint8_t* img;      // (F, h, w, 3) or NULL
    const float* flow;       // (F, h, w, 2) or NULL
    const float* occ;        // (F, h, w) or NULL
    const void* mask;        // (F, h, w) fp32 / uint8 or NULL
    const int* dp;           // (F, h, w) or NULL
    const double* aff;       // (F, 4), in OUTPUT order
    float *o_img, *o_flow, *o_occ, *o_mask, *o_dp, *o_vis;
    int F, bs, h, w, S, mask_u8;
};

__global__ __launch_bounds__(kBlock) void crop_remap_kernel(CropArgs a) {
    const int o = blockIdx.y;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const int S = a.S, SS = S * S;
    if (p >= SS) return;
    const int row = p / S, col = p - row * S;
    const int f = src_frame(o, a.bs);
    const double a0 = a.aff[o * 4 + 0], a1 = a.aff[o * 4 + 1], tx = a.aff[o * 4 + 2], ty = a.aff[o * 4 + 3];
    const bool live = a0 == a0;                                            // a refused frame: zeros, nothing read
    const float x = (float)((double)col * a0 + tx), y = (float)((double)row * a1 + ty);
    const int64_t hw = (int64_t)a.h * a.w, fo = (int64_t)o * SS + p;
    Taps t = linear_taps(x, y);
    t.ok = t.ok && live;
    int xi = 0, yi = 0;
    const bool in = live && nearest_px(x, y, a.w, a.h, xi, yi);
    const int64_t np = (int64_t)yi * a.w + xi;
    if (a.o_img) {
        const uint8_t* s = a.img + f * hw * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.o_img[((int64_t)o * 3 + c) * SS + p] = blend(s + c, 3, a.w, a.h, t, 255.0f);
    }
    if (a.o_flow) {
        const float* s = a.flow + f * hw * 2;
#pragma unroll
        for (int c = 0; c < 2; ++c) a.o_flow[((int64_t)o * 2 + c) * SS + p] = blend(s + c, 2, a.w, a.h, t, 0.0f);
    }
    if (a.o_occ) a.o_occ[fo] = blend(a.occ + f * hw, 1, a.w, a.h, t, 0.0f);
    if (a.o_vis) a.o_vis[fo] = in ? 1.0f : 0.0f;
    if (a.o_mask) {
        bool on = false;
        if (in) on = a.mask_u8 ? ((const uint8_t*)a.mask)[f * hw + np] > 0 : ((const float*)a.mask)[f * hw + np] > 0.0f;
        a.o_mask[fo] = on ? 1.0f : 0.0f;                                   // (mask * vis2d) > 0: vis2d is 1 wherever `in`
    }
    if (a.o_dp) a.o_dp[fo] = in ? (float)a.dp[f * hw + np] : 0.0f;
}

// ---- flow_process -----------------------------------------------------------------------------------------------------------
// the flow of frame `me` at pixel (col, row), re-expressed in the crop of the other frame (affine ao), rounded to fp32 as the
// reference stores it
DEVINL void screen_flow(const float* __restrict__ fl, int SS, int p, int col, int row, const double* am, const double* ao, float& fx,
                        float& fy) {
    const double hx = (double)col * am[0] + am[2], hy = (double)row * am[1] + am[3];
    fx = (float)((((double)fl[p] + hx) - ao[2]) / ao[0] - (double)col);
    fy = (float)((((double)fl[SS + p] + hy) - ao[3]) / ao[1] - (double)row);
}

__global__ __launch_bounds__(kBlock) void flow_process_kernel(const float* __restrict__ flow_c, const double* __restrict__ aff, int bs,
                                                             int S, float* __restrict__ flow, float* __restrict__ occ) {
    const int o = blockIdx.y, q = partner(o, bs);
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const int SS = S * S;
    if (p >= SS) return;
    const int row = p / S, col = p - row * S;
    double am[4], ao[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        am[k] = aff[o * 4 + k];
        ao[k] = aff[q * 4 + k];
    }
    float* fo = flow + (int64_t)o * 2 * SS;
    if (!(am[0] == am[0]) || !(ao[0] == ao[0])) {                          // a refused frame in the pair: zeros for both
        fo[p] = 0.0f;
        fo[SS + p] = 0.0f;
        occ[(int64_t)o * SS + p] = 0.0f;
        return;
    }
    float fx, fy;
    screen_flow(flow_c + (int64_t)o * 2 * SS, SS, p, col, row, am, ao, fx, fy);
    // warp_flow: the map is formed in fp32
    const Taps t = linear_taps(fx + (float)col, fy + (float)row);
    double rx = 0.0, ry = 0.0;
    if (t.ok) {
        const float* fq = flow_c + (int64_t)q * 2 * SS;
        const float wt[4] = {t.w00, t.w01, t.w10, t.w11};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xi = t.x0 + (k & 1), yi = t.y0 + (k >> 1);
            double vx = 0.0, vy = 0.0;                                     // a tap outside the image is the constant 0
            if (xi >= 0 && xi < S && yi >= 0 && yi < S) {
                float gx, gy;
                screen_flow(fq, SS, yi * S + xi, xi, yi, ao, am, gx, gy);
                vx = (double)xi + (double)gx;
                vy = (double)yi + (double)gy;
            }
            rx = rx + vx * (double)wt[k];
            ry = ry + vy * (double)wt[k];
        }
    }
    const double dx = rx - (double)col, dy = ry - (double)row;
    const double dis = sqrt(dx * dx + dy * dy);
    double oc = exp(-25.0 * (dis / (double)S * 2.0));
    if (oc < 0.25) oc = 0.0;
    occ[(int64_t)o * SS + p] = (float)oc;
    fo[p] = 2.0f * (fx / (float)S);
    fo[SS + p] = 2.0f * (fy / (float)S);
}

// ---- remap with explicit maps -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void remap_kernel(const float* __restrict__ src, int C, int Hs, int Ws,
                                                      const float* __restrict__ map_x, const float* __restrict__ map_y, int64_t n,
                                                      int linear, float* __restrict__ dst) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n) return;
    const float x = map_x[p], y = map_y[p];
    const int64_t plane = (int64_t)Hs * Ws;
    if (linear) {
        const Taps t = linear_taps(x, y);
        for (int c = 0; c < C; ++c) dst[c * n + p] = blend(src + c * plane, 1, Ws, Hs, t, 0.0f);
    } else {
        int xi = 0, yi = 0;
        const bool in = nearest_px(x, y, Ws, Hs, xi, yi);
        for (int c = 0; c < C; ++c) dst[c * n + p] = in ? src[c * plane + (int64_t)yi * Ws + xi] : 0.0f;
    }
}

bool frame_ok(int64_t B, int64_t h, int64_t w) {
    return B >= 1 && h >= 1 && w >= 1 && h < 32768 && w < 32768 && (double)h * w < 1073741824.0 && B < (1 << 16);
}

}   // namespace

extern "C" int moda_mask_bbox(const void* masks, int32_t is_u8, int64_t B, int64_t h, int64_t w, int32_t* box, void* stream) {
    if (!frame_ok(B, h, w)) return MODA_ESHAPE;
    if (!masks || !box) return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bbox_init_kernel, dim3(nblocks(B, kBlock)), dim3(kBlock), 0, st, box, (int)B, (int)h, (int)w);
    unsigned nb = nblocks(h * w, kBlock * 16);
    nb = nb < 1 ? 1 : (nb > kBboxMaxBlocks ? kBboxMaxBlocks : nb);
    if (is_u8)
        hipLaunchKernelGGL(bbox_kernel<true>, dim3(nb, (unsigned)B), dim3(kBlock), 0, st, masks, (int)h, (int)w, box);
    else
        hipLaunchKernelGGL(bbox_kernel<false>, dim3(nb, (unsigned)B), dim3(kBlock), 0, st, masks, (int)h, (int)w, box);
    return (int)hipGetLastError();
}

extern "C" int moda_crop_params(const int32_t* box, int64_t B, int64_t bs, int64_t img_size, double crop_factor, float* kaug,
                                double* affine, int32_t* status, void* stream) {
    if (B < 1 || B >= (1 << 16) || img_size < 1 || img_size > 16384 || bs < 0 || (bs > 0 && B != 2 * bs)) return MODA_ESHAPE;
    if (!box || !kaug || !affine || !(crop_factor > 0.0) || !(crop_factor < 1024.0)) return MODA_EINVAL;
    hipLaunchKernelGGL(crop_params_kernel, dim3(nblocks(B, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, box, (int)B, (int)bs,
                       (int)img_size, crop_factor, kaug, affine, status);
    return (int)hipGetLastError();
}

extern "C" int moda_crop_remap(const uint8_t* img, const float* flow, const float* occ, const void* mask, int32_t mask_u8,
                               const int32_t* dp, const double* affine, int64_t B, int64_t bs, int64_t h, int64_t w, int64_t img_size,
                               float* o_img, float* o_flow, float* o_occ, float* o_mask, float* o_dp, float* o_vis, void* stream) {
    if (!frame_ok(B, h, w) || img_size < 1 || img_size > 16384 || bs < 0 || (bs > 0 && B != 2 * bs)) return MODA_ESHAPE;
    if ((double)B * 3 * img_size * img_size >= 2147483648.0 * 4) return MODA_ESHAPE;
    if (!affine || (o_img && !img) || (o_flow && !flow) || (o_occ && !occ) || (o_mask && !mask) || (o_dp && !dp)) return MODA_EINVAL;
    CropArgs a = {img,   flow,  occ,   mask,   dp,    affine,  o_img,  o_flow,       o_occ,        o_mask,
                  o_dp,  o_vis, (int)B, (int)bs, (int)h, (int)w, (int)img_size, mask_u8 ? 1 : 0};
    hipLaunchKernelGGL(crop_remap_kernel, dim3(nblocks(img_size * img_size, kBlock), (unsigned)B), dim3(kBlock), 0, (hipStream_t)stream,
                       a);
    return (int)hipGetLastError();
}

extern "C" int moda_flow_process(const float* flow_c, const double* affine, int64_t bs, int64_t img_size, float* flow, float* occ,
                                 void* stream) {
    if (bs < 1 || bs >= (1 << 15) || img_size < 1 || img_size > 16384) return MODA_ESHAPE;
    if ((double)bs * 4 * img_size * img_size >= 2147483648.0 * 4) return MODA_ESHAPE;
    if (!flow_c || !affine || !flow || !occ || flow == flow_c) return MODA_EINVAL;
    hipLaunchKernelGGL(flow_process_kernel, dim3(nblocks(img_size * img_size, kBlock), (unsigned)(2 * bs)), dim3(kBlock), 0,
                       (hipStream_t)stream, flow_c, affine, (int)bs, (int)img_size, flow, occ);
    return (int)hipGetLastError();
}

extern "C" int moda_remap(const float* src, int64_t C, int64_t Hs, int64_t Ws, const float* map_x, const float* map_y, int64_t H,
                          int64_t W, int32_t interpolation, float* dst, void* stream) {
    if (!frame_ok(1, Hs, Ws) || C < 1 || C > 65536 || H < 1 || W < 1 || (double)H * W >= 1073741824.0) return MODA_ESHAPE;
    if ((double)C * H * W >= 4.0e9 || (double)C * Hs * Ws >= 4.0e9) return MODA_ESHAPE;
    if (!src || !map_x || !map_y || !dst) return MODA_EINVAL;
    if (interpolation != MODA_REMAP_NEAREST && interpolation != MODA_REMAP_LINEAR) return MODA_EINVAL;
    hipLaunchKernelGGL(remap_kernel, dim3(nblocks(H * W, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, src, (int)C, (int)Hs, (int)Ws,
                       map_x, map_y, H * W, interpolation == MODA_REMAP_LINEAR ? 1 : 0, dst);
    return (int)hipGetLastError();
}
