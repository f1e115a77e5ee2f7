// The pose CNN in inference mode (reference nnutils/nerf.py:513-573: ResNetConv = the ResNet-18 trunk, Encoder = trunk + one
// 3x3 conv block + max_pool2d(4, 4)), as it is run by extract_cams / eval_cam (nnutils/train_utils.py:393-453, 794-807).  fp32 only.
//
//   conv2d_nhwc  implicit-GEMM convolution on v_mfma_f32_32x32x2_f32: rows = output pixels (b, oy, ox), columns = output channels,
//                K = (ky, kx, c) with c fastest -- the order in which an NHWC input holds a tap and in which the weights are packed
//                ([Cout][kh][kw][Cin]).  K is walked in chunks of 16 channels of one tap (Cin % 16 == 0): a workgroup stages the
//                chunk of its pixels and of its output channels in LDS as 16 planes (k-major, so that an operand read is one
//                conflict-free 4-byte read per lane), every wave owns one 32 x 32 tile and chains 8 MFMAs per chunk; the next
//                chunk's global loads are issued before those MFMAs and written to LDS after them.  A tap outside the image is
//                a zero operand, never a skipped step.  Two forms: 2 x 2 waves (64 pixels x 64 channels per workgroup) where that
//                gives at least one workgroup per CU, else one wave per workgroup (32 x 32), which is what the 4 x 4 maps of
//                layer 4 and the tail get their parallelism from.
//   bits         every output element is ONE fp32 fma chain over k = 0 .. K-1 in ascending order, started from 0 (the MFMA is
//                bit for bit that chain, one rounding per step), then + bias, + residual, activation, each one rounded fp32
//                operation.  No split of K, no atomics.  The chain does not depend on the tile form, on the element's place in a
//                tile or in the grid, or on how many other pixels the launch has: a frame has the same bits alone and in any batch.
//   maxpool      3 x 3, stride 2, padding 1 over NHWC with torch's semantics: the padding is -inf, a NaN wins.
//   input        NCHW (B,C,H,W) -> NHWC (B,H,W,Cp), channels C .. Cp-1 zero; optionally x / max(|x|_2, 1e-12) over the C channels
//                (F.normalize(., 2, 1)), the norm formed in float64 so that the result is the correctly rounded quotient of the
//                float64 formula up to the final fp32 rounding.
//   tail         (B,P,C) -> (B,C): the maximum over the P positions (max_pool2d over the whole 4 x 4 map), a NaN wins.
// Device memory is written only by plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBlock = 256;
constexpr int kKC = MODA_CONV_K_CHUNK;           // channels of one tap per LDS stage
constexpr int kBigTilesWanted = 256;             // the 64 x 64 form needs one workgroup per CU

struct ConvArgs {
    const float* in;
    const float* w;
    const float* bias;
    const float* res;
    float* out;
    int64_t M;                                   // B * Ho * Wo
    int H, W, Cin, Cout, Ho, Wo, kh, kw, stride, pad, act;
};

DEVINL float activate(float v, int act) {
    if (act == MODA_CONV_ACT_RELU) return v < 0.0f ? 0.0f : v;                 // NaN stays NaN, as torch's relu
    if (act == MODA_CONV_ACT_LEAKY) return v > 0.0f ? v : v * 0.2f;
    return v;
}

template <int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void conv2d_nhwc_kernel(ConvArgs a) {
    constexpr int NT = 64 * WM * WN, BM = 32 * WM, BN = 32 * WN;
    constexpr int SA = (BM % 64 == 32) ? BM : BM + 32;                         // plane stride = 32 (mod 64): the two k of a step, held by
    constexpr int SB = (BN % 64 == 32) ? BN : BN + 32;                         // the two lane halves, fall into opposite bank halves
    constexpr int NA = BM * 4 / NT, NB = BN * 4 / NT;                          // float4 loads per thread and chunk
    static_assert(NT % BM == 0 && NT % BN == 0 && NA >= 1 && NB >= 1, "a thread keeps its row");
    __shared__ float As[kKC * SA];
    __shared__ float Bs[kKC * SB];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, wm = wv % WM, wn = wv / WM, col = lane & 31, h = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int K = a.kh * a.kw * a.Cin, cpt = a.Cin / kKC, nchunks = K / kKC;

    // the pixel whose chunk rows this thread stages, and the output channel
    const int arow = t % BM, akq = t / BM, brow = t % BN, bkq = t / BN;
    const int64_t m = m0 + arow;
    const bool a_ok = m < a.M;
    const int64_t mm = a_ok ? m : 0;
    const int per_img = a.Ho * a.Wo;
    const int64_t b = mm / per_img;
    const int rem = (int)(mm - b * per_img), oy = rem / a.Wo, ox = rem - oy * a.Wo;
    const int iy0 = oy * a.stride - a.pad, ix0 = ox * a.stride - a.pad;
    const float* inb = a.in + b * (int64_t)a.H * a.W * a.Cin;
    const int n = n0 + brow;
    const bool b_ok = n < a.Cout;
    const float* wrow = a.w + (int64_t)(b_ok ? n : 0) * K;

    float4 ra[NA], rb[NB];
    auto fetch = [&](int kc) {
        const int tap = kc / cpt, c0 = (kc - tap * cpt) * kKC, ky = tap / a.kw, kx = tap - ky * a.kw;
        const int iy = iy0 + ky, ix = ix0 + kx;
        const bool ok = a_ok && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const float* p = inb + ((int64_t)(ok ? iy : 0) * a.W + (ok ? ix : 0)) * a.Cin + c0;
#pragma unroll
        for (int i = 0; i < NA; ++i)
            ra[i] = ok ? *(const float4*)(p + 4 * (akq + i * (NT / BM))) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < NB; ++i)
            rb[i] = b_ok ? *(const float4*)(wrow + (int64_t)kc * kKC + 4 * (bkq + i * (NT / BN))) : make_float4(0.f, 0.f, 0.f, 0.f);
    };

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

    fetch(0);
    for (int kc = 0; kc < nchunks; ++kc) {
        __syncthreads();                                                       // the previous chunk has been read
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int k = 4 * (akq + i * (NT / BM));
            As[(k + 0) * SA + arow] = ra[i].x;
            As[(k + 1) * SA + arow] = ra[i].y;
            As[(k + 2) * SA + arow] = ra[i].z;
            As[(k + 3) * SA + arow] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int k = 4 * (bkq + i * (NT / BN));
            Bs[(k + 0) * SB + brow] = rb[i].x;
            Bs[(k + 1) * SB + brow] = rb[i].y;
            Bs[(k + 2) * SB + brow] = rb[i].z;
            Bs[(k + 3) * SB + brow] = rb[i].w;
        }
        __syncthreads();
        if (kc + 1 < nchunks) fetch(kc + 1);                                   // in flight under the MFMAs
#pragma unroll
        for (int s = 0; s < kKC / 2; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * s + h) * SA + wm * 32 + col], Bs[(2 * s + h) * SB + wn * 32 + col], acc,
                                                       0, 0, 0);
    }

    const int no = n0 + wn * 32 + col;
    if (no < a.Cout) {
        const float bv = a.bias[no];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t mo = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;  // the accumulator's row
            if (mo < a.M) {
                const int64_t o = mo * a.Cout + no;
                float v = acc[r] + bv;
                if (a.res) v = v + a.res[o];
                a.out[o] = activate(v, a.act);
            }
        }
    }
}

// one thread per (output pixel, 4 channels)
__global__ __launch_bounds__(kBlock) void maxpool3x3s2_kernel(const float* __restrict__ in, int64_t total, int H, int W, int C4, int Ho,
                                                             int Wo, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    int64_t p = i / C4;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho);
    const int64_t b = p / Ho;
    const float ninf = -__builtin_inff();
    float4 mx = make_float4(ninf, ninf, ninf, ninf);
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            const float4 v = ((const float4*)in)[((b * H + iy) * W + ix) * C4 + c4];
            if (v.x > mx.x || v.x != v.x) mx.x = v.x;                          // torch: (val > max) || isnan(val)
            if (v.y > mx.y || v.y != v.y) mx.y = v.y;
            if (v.z > mx.z || v.z != v.z) mx.z = v.z;
            if (v.w > mx.w || v.w != v.w) mx.w = v.w;
        }
    }
    ((float4*)out)[i] = mx;
}

// one thread per pixel: C strided reads (coalesced over the lanes), Cp contiguous writes
__global__ __launch_bounds__(kBlock) void posecnn_input_kernel(const float* __restrict__ src, int64_t npix, int64_t HW, int C, int Cp,
                                                              int normalize, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= npix) return;
    const int64_t b = i / HW, p = i - b * HW;
    const float* s = src + b * C * HW + p;
    double inv = 1.0;
    if (normalize) {
        double ss = 0.0;
        for (int c = 0; c < C; ++c) {
            const double v = (double)s[(int64_t)c * HW];
            ss = __builtin_fma(v, v, ss);
        }
        const double nrm = __builtin_sqrt(ss);
        inv = nrm > 1e-12 ? nrm : 1e-12;                                       // F.normalize: v / max(|v|, eps)
        if (nrm != nrm) inv = nrm;                                             // a NaN norm stays NaN, as torch's clamp_min keeps it
    }
    float* d = dst + i * Cp;
    for (int c = 0; c < Cp; ++c) {
        float v = 0.0f;
        if (c < C) {
            v = s[(int64_t)c * HW];
            if (normalize) v = (float)((double)v / inv);
        }
        d[c] = v;
    }
}

// one thread per (b, c)
__global__ __launch_bounds__(kBlock) void posecnn_tail_kernel(const float* __restrict__ x, int64_t total, int P, int C, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / C;
    const int c = (int)(i - b * C);
    float mx = -__builtin_inff();
    for (int p = 0; p < P; ++p) {
        const float v = x[(b * P + p) * C + c];
        if (v > mx || v != v) mx = v;
    }
    out[i] = mx;
}

}   // namespace

extern "C" int32_t moda_conv2d_tile(int64_t M, int64_t Cout, int32_t tile) {
    if (tile == MODA_CONV_TILE_32 || tile == MODA_CONV_TILE_64) return tile;
    if (M < 1 || Cout < 1) return MODA_CONV_TILE_32;
    return (double)((M + 63) / 64) * (double)((Cout + 63) / 64) >= (double)kBigTilesWanted ? MODA_CONV_TILE_64 : MODA_CONV_TILE_32;
}

extern "C" int moda_conv2d_nhwc(const float* in, const float* w, const float* bias, const float* res, float* out, int64_t B, int64_t H,
                                int64_t W, int64_t Cin, int64_t Cout, int32_t kh, int32_t kw, int32_t stride, int32_t pad, int32_t act,
                                int32_t tile, void* stream) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || kh < 1 || kw < 1 || stride < 1 || pad < 0) return MODA_ESHAPE;
    if (Cin % kKC != 0 || kh > 16 || kw > 16 || stride > 16 || pad >= kh || pad >= kw || H > 32768 || W > 32768 || Cin > 65536 ||
        Cout > 65536)
        return MODA_ESHAPE;
    if (H + 2 * pad < kh || W + 2 * pad < kw) return MODA_ESHAPE;
    const int64_t Ho = (H + 2 * pad - kh) / stride + 1, Wo = (W + 2 * pad - kw) / stride + 1;
    if ((double)B * H * W * Cin >= 2147483648.0 * 4 || (double)B * Ho * Wo * Cout >= 2147483648.0 * 4 || (double)B * Ho * Wo >= 2147483648.0)
        return MODA_ESHAPE;
    if (act != MODA_CONV_ACT_NONE && act != MODA_CONV_ACT_RELU && act != MODA_CONV_ACT_LEAKY) return MODA_EINVAL;
    if (tile != MODA_CONV_TILE_AUTO && tile != MODA_CONV_TILE_32 && tile != MODA_CONV_TILE_64) return MODA_EINVAL;
    if (!in || !w || !bias || !out || !al16(in) || !al16(w)) return MODA_EINVAL;
    ConvArgs a;
    a.in = in; a.w = w; a.bias = bias; a.res = res; a.out = out;
    a.M = B * Ho * Wo;
    a.H = (int)H; a.W = (int)W; a.Cin = (int)Cin; a.Cout = (int)Cout; a.Ho = (int)Ho; a.Wo = (int)Wo;
    a.kh = kh; a.kw = kw; a.stride = stride; a.pad = pad; a.act = act;
    hipStream_t st = (hipStream_t)stream;
    if (moda_conv2d_tile(a.M, Cout, tile) == MODA_CONV_TILE_64)
        hipLaunchKernelGGL((conv2d_nhwc_kernel<2, 2>), dim3(nblocks(a.M, 64), nblocks(Cout, 64)), dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((conv2d_nhwc_kernel<1, 1>), dim3(nblocks(a.M, 32), nblocks(Cout, 32)), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}

extern "C" int moda_maxpool3x3s2_nhwc(const float* in, int64_t B, int64_t H, int64_t W, int64_t C, float* out, void* stream) {
    if (B < 1 || H < 1 || W < 1 || C < 1 || C % 4 != 0) return MODA_ESHAPE;
    const int64_t Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    if ((double)B * H * W * C >= 2147483648.0 * 4 || H > 32768 || W > 32768) return MODA_ESHAPE;
    if (!in || !out || !al16(in) || !al16(out)) return MODA_EINVAL;
    const int64_t total = B * Ho * Wo * (C / 4);
    hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3(nblocks(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, in, total, (int)H, (int)W,
                       (int)(C / 4), (int)Ho, (int)Wo, out);
    return (int)hipGetLastError();
}

extern "C" int moda_posecnn_input(const float* src, int64_t B, int64_t C, int64_t H, int64_t W, int64_t Cp, int32_t normalize, float* dst,
                                  void* stream) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || Cp < C || Cp > 65536) return MODA_ESHAPE;
    if ((double)B * H * W * Cp >= 2147483648.0 * 4 || (double)B * H * W >= 2147483648.0) return MODA_ESHAPE;
    if (!src || !dst) return MODA_EINVAL;
    hipLaunchKernelGGL(posecnn_input_kernel, dim3(nblocks(B * H * W, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, src, B * H * W, H * W,
                       (int)C, (int)Cp, normalize, dst);
    return (int)hipGetLastError();
}

extern "C" int moda_posecnn_tail(const float* x, int64_t B, int64_t P, int64_t C, float* out, void* stream) {
    if (B < 1 || P < 1 || C < 1 || P > 65536 || C > 65536 || (double)B * P * C >= 2147483648.0 * 4) return MODA_ESHAPE;
    if (!x || !out) return MODA_EINVAL;
    hipLaunchKernelGGL(posecnn_tail_kernel, dim3(nblocks(B * C, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, x, B * C, (int)P, (int)C,
                       out);
    return (int)hipGetLastError();
}
