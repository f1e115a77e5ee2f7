// Evaluation-frame kernels (include/moda_hip_vis.h): what v2s_trainer.eval() does to the rendered frames of a chunk between
// render_rays and the written pictures -- the masked, normalised canvases of train_utils.py:496-520, image_grid, add_image's
// display forms, flow_to_image and save_vid's 8-bit frames -- without a host read.
//
//   * extrema: ONE two-stage reduction over a table of keys.  Floats are mapped to integers that order as they do (-0 below +0,
//     every NaN canonical and above +inf), and the minimum is the maximum of the negated values, so both stages are integer
//     maxima: exact, associative and commutative, hence the same bits for every tiling and on every run.  No float atomics.
//   * canvases: one pass over all keys of a chunk, driven by the same table: nearest-resized mask, product, x - min, * 255 / max.
//   * flow colours: the reference's arithmetic at the reference's precisions (see moda_flow_color in the header).
//   * grid, frame pick and 8-bit conversion are gathers: one thread per output element, consecutive lanes store consecutive
//     addresses.
// Contraction is off for the whole file: numpy and torch round every product and sum on their own.
#include "lanes.h"
#include "moda_hip_vis.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = MODA_VIS_BLOCK;
constexpr int kTile = MODA_VIS_TILE;
constexpr int kWaves = kBlock / 64;
constexpr int kLowest = (int)0x80000000;        // below ord(-inf): the neutral element of the integer maximum

struct VisOp { long long off, n, C, flags, mul_off, r0, r1, r2; };
static_assert(sizeof(VisOp) == 8 * MODA_VIS_OP_FIELDS, "an op-table row is MODA_VIS_OP_FIELDS int64");

struct VisMask { const float* m; long long bs; int Sm, S; float scale; };

DEVINL int ord(float f) {
    const int b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
DEVINL float unord(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }
DEVINL float canon(float f) { return f != f ? __int_as_float(0x7fc00000) : f; }
DEVINL float qnan() { return __int_as_float(0x7fc00000); }

// a row that the kernels follow: inside the packed buffer, channel count and lengths sane
DEVINL bool op_ok(const VisOp& op, long long total, int tiles, bool reduce_only) {
    if (op.n > (long long)tiles * kTile) return false;          // beyond the grid and the partials the caller sized
    if (op.n < 1 || op.C < 1 || op.off < 0 || op.n > 0x7fffffffLL || op.C > 65536) return false;
    const bool rad = op.flags & MODA_VIS_OP_RAD;
    if (rad && (!reduce_only || op.C < 2)) return false;
    const long long len = rad ? op.n * op.C : op.n;
    if (op.off > total - len) return false;
    if (!rad && op.n % op.C) return false;
    if ((op.flags & MODA_VIS_OP_MUL) && (op.mul_off < 0 || op.mul_off > total - op.n / op.C)) return false;
    return true;
}

// the value of element e of a key (header: moda_vis_minmax)
DEVINL float vis_value(const float* __restrict__ x, const VisOp& op, long long e, const VisMask& mk) {
    if (op.flags & MODA_VIS_OP_RAD) {
        float u = x[op.off + e * op.C], v = x[op.off + e * op.C + 1];
        if (fabsf(u) > 1e7f || fabsf(v) > 1e7f) u = v = 0.f;
        return sqrtf(u * u + v * v);
    }
    float val = x[op.off + e];
    const long long p = e / op.C;
    if (op.flags & MODA_VIS_OP_MASK) {
        float m = qnan();
        if (mk.m) {
            const long long SS = (long long)mk.S * mk.S, b = p / SS;
            const int pix = (int)(p - b * SS), y = pix / mk.S, xx = pix - y * mk.S;
            const int ys = min((int)floorf(y * mk.scale), mk.Sm - 1), xs = min((int)floorf(xx * mk.scale), mk.Sm - 1);
            if (b < mk.bs) m = mk.m[(b * mk.Sm + ys) * mk.Sm + xs];
        }
        val = val * m;
    }
    if (op.flags & MODA_VIS_OP_MUL) val = val * x[op.mul_off + p];
    return val;
}

// the integer maxima of a workgroup: every lane's (a, b) -> valid in thread 0
DEVINL void block_max2(int& a, int& b, int (*lds)[2]) {
    auto mx = [](int p, int q) { return p > q ? p : q; };
    a = wave_all(a, mx);
    b = wave_all(b, mx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { lds[wave][0] = a; lds[wave][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) { a = mx(a, lds[w][0]); b = mx(b, lds[w][1]); }
    }
}

// stage 1: grid (tiles, nkeys); part[(key tiles + tile)] = [ord-max of -value, ord-max of value] of the tile
__global__ __launch_bounds__(kBlock) void vis_minmax_tiles(const float* __restrict__ x, long long total, const VisOp* __restrict__ ops,
                                                           VisMask mk, int tiles, int* __restrict__ part) {
    __shared__ int lds[kWaves][2];
    const VisOp op = ops[blockIdx.y];
    if (!op_ok(op, total, tiles, true)) return;                          // workgroup-uniform
    const long long base = (long long)blockIdx.x * kTile;
    if (base >= op.n) return;
    int kmin = kLowest, kmax = kLowest;
#pragma unroll
    for (int i = 0; i < kTile / kBlock; ++i) {
        const long long e = base + i * kBlock + threadIdx.x;
        if (e < op.n) {
            const float v = vis_value(x, op, e, mk);
            kmax = max(kmax, ord(canon(v)));
            kmin = max(kmin, ord(canon(-v)));
        }
    }
    block_max2(kmin, kmax, lds);
    if (threadIdx.x == 0) {
        int* o = part + ((long long)blockIdx.y * tiles + blockIdx.x) * 2;
        o[0] = kmin;
        o[1] = kmax;
    }
}

// stage 2: one workgroup a key over its tiles' partials -> mm[key] = [min, max]; the key's status counts
__global__ __launch_bounds__(kBlock) void vis_minmax_keys(const VisOp* __restrict__ ops, long long total, int tiles,
                                                          const int* __restrict__ part, float* __restrict__ mm, int* __restrict__ status) {
    __shared__ int lds[kWaves][2];
    const VisOp op = ops[blockIdx.x];
    const bool ok = op_ok(op, total, tiles, true);
    int kmin = kLowest, kmax = kLowest;
    if (ok) {
        const int nt = (int)((op.n + kTile - 1) / kTile);
        for (int t = threadIdx.x; t < nt; t += kBlock) {
            const int* p = part + ((long long)blockIdx.x * tiles + t) * 2;
            kmin = max(kmin, p[0]);
            kmax = max(kmax, p[1]);
        }
    }
    block_max2(kmin, kmax, lds);
    if (threadIdx.x == 0) {
        const float mn = ok ? -unord(kmin) : qnan(), mx = ok ? unord(kmax) : qnan();
        mm[2 * blockIdx.x] = mn;
        mm[2 * blockIdx.x + 1] = mx;
        if (mn != mn || mx != mx) atomicAdd(status + MODA_VIS_STATUS_NAN_EXT, 1);
        const bool sub = op.flags & (MODA_VIS_OP_SUBMIN | MODA_VIS_OP_UNIT);
        if ((op.flags & (MODA_VIS_OP_SCALE255 | MODA_VIS_OP_UNIT)) && (sub ? mx - mn : mx) == 0.f)
            atomicAdd(status + MODA_VIS_STATUS_ZERO_DIV, 1);
    }
}

// the canvas pass: grid (tiles, nkeys), one element a lane and step
__global__ __launch_bounds__(kBlock) void vis_apply_kernel(const float* __restrict__ x, long long total, const VisOp* __restrict__ ops,
                                                           VisMask mk, const float* __restrict__ mm, float* __restrict__ out) {
    const VisOp op = ops[blockIdx.y];
    if (!op_ok(op, total, (int)gridDim.x, false)) return;
    const long long base = (long long)blockIdx.x * kTile;
    if (base >= op.n) return;
    const float mn = mm[2 * blockIdx.y], mx = mm[2 * blockIdx.y + 1];
    // SUBMIN / SCALE255 are formed in float64 from the fp32 value and extrema and rounded ONCE: the reference rounds x - min,
    // max - min, 255 / d and the product to fp32 each, which leaves it up to 2.2 ulp from the float64 value; this is within 0.5
    const double dmn = (op.flags & MODA_VIS_OP_SUBMIN) ? (double)mn : 0.0;
    const double scale = (op.flags & MODA_VIS_OP_SCALE255) ? 255.0 / ((double)mx - dmn) : 1.0;
    const float len = mx - mn;
#pragma unroll
    for (int i = 0; i < kTile / kBlock; ++i) {
        const long long e = base + i * kBlock + threadIdx.x;
        if (e >= op.n) break;
        float v = vis_value(x, op, e, mk);
        if (op.flags & (MODA_VIS_OP_SUBMIN | MODA_VIS_OP_SCALE255)) v = (float)(((double)v - dmn) * scale);
        if (op.flags & MODA_VIS_OP_UNIT) v = (v - mn) / len;
        if (op.flags & MODA_VIS_OP_CLAMP01) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
        out[op.off + e] = v;
    }
}

// flow_to_image: grid (ceil(HW / kBlock), N).  T: the precision of u, v, radius, angle and fk after the normalisation.
template <class T>
__global__ __launch_bounds__(kBlock) void flow_color_kernel(const float* __restrict__ flow, int HW, int C, const float* __restrict__ maxrad,
                                                            const float* __restrict__ wheel, uint8_t* __restrict__ out) {
    __shared__ float wh[55 * 3];
    if (threadIdx.x < 55 * 3) wh[threadIdx.x] = wheel[threadIdx.x];
    __syncthreads();
    const int p = blockIdx.x * kBlock + threadIdx.x;
    if (p >= HW) return;
    const long long px = (long long)blockIdx.y * HW + p;
    float u = flow[px * C], v = flow[px * C + 1];
    const bool unknown = fabsf(u) > 1e7f || fabsf(v) > 1e7f;
    if (unknown) u = v = 0.f;
    const float mr = maxrad[blockIdx.y];
    T den;
    if (mr != mr) den = sizeof(T) == 8 ? (T)(-1.0 + 2.220446049250313e-16) : (T)-1;                 // max(-1, nan) is -1
    else if (sizeof(T) == 8) den = (T)((double)mr + 2.220446049250313e-16);
    else den = (T)(mr + 2.220446e-16f);
    T ud = (T)u / den, vd = (T)v / den;
    const bool isnan_ = ud != ud || vd != vd;
    if (isnan_) ud = vd = (T)0;
    const T rad = sqrt(ud * ud + vd * vd);
    const T a = atan2(-vd, -ud) / (T)3.141592653589793;
    const T fk = (a + (T)1) / (T)2 * (T)54 + (T)1;
    int k0 = (int)floor(fk);
    k0 = k0 < 1 ? 1 : (k0 > 55 ? 55 : k0);                       // fk lies in [1, 55]: the clamp only keeps the table read inside
    const int k1 = k0 == 55 ? 1 : k0 + 1;
    const double f = (double)fk - (double)k0;
    uint8_t* o = out + px * 3;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double c0 = (double)wh[(k0 - 1) * 3 + i] / 255.0, c1 = (double)wh[(k1 - 1) * 3 + i] / 255.0;
        double col = (1.0 - f) * c0 + f * c1;
        if (rad <= (T)1) col = 1.0 - (double)rad * (1.0 - col);
        else col = col * 0.75;
        double lvl = floor(255.0 * col * (isnan_ ? 0.0 : 1.0));
        lvl = lvl < 0.0 ? 0.0 : (lvl > 255.0 ? 255.0 : lvl);     // col lies in [0, 1]
        o[i] = unknown ? (uint8_t)0 : (uint8_t)(int)lvl;
    }
}

__global__ __launch_bounds__(kBlock) void vis_grid_kernel(const float* __restrict__ img, int h, int w, int c, int col, int total,
                                                          float* __restrict__ out) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= total) return;
    const int line = col * w * c, Y = e / line, r = e - Y * line, X = r / c, cc = r - X * c;
    const int i = Y / h, y = Y - i * h, j = X / w, x = X - j * w;
    out[e] = img[(((long long)(i * col + j) * h + y) * w + x) * c + cc];
}

__global__ __launch_bounds__(kBlock) void vis_to_u8_kernel(const float* __restrict__ frames, int N, int E, const int* __restrict__ pick,
                                                           long long total, const float* __restrict__ mm, uint8_t* __restrict__ out,
                                                           int* __restrict__ status) {
    const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
    bool sat = false, nan = false;
    if (e < total) {
        const long long i = e / E;
        const int f = pick[i];
        float v = 0.f;
        if (f >= 0 && f < N) {
            v = frames[(long long)f * E + (e - i * E)];
            if (mm && mm[2 * f + 1] <= 1.f) v = v * 255.f;
        }
        nan = v != v;
        sat = v <= -1.f || v >= 256.f;
        const float t = nan ? 0.f : truncf(fminf(fmaxf(v, 0.f), 255.f));
        out[e] = (uint8_t)(int)t;
    }
    const int ns = __popcll(__ballot(sat)), nn = __popcll(__ballot(nan));      // all lanes reach this
    if ((threadIdx.x & 63) == 0) {
        if (ns) atomicAdd(status + MODA_VIS_STATUS_SATURATED, ns);
        if (nn) atomicAdd(status + MODA_VIS_STATUS_NAN_U8, nn);
    }
}

int table_shape(int64_t total, int64_t nkeys, int64_t max_n, const float* mask, int64_t mask_bs, int64_t Sm, int64_t S, VisMask* mk) {
    if (nkeys < 1 || nkeys > MODA_VIS_MAX_KEYS || max_n < 1 || max_n > 0x7fffffffLL || total < 1 || total > 0x7fffffffLL) return MODA_ESHAPE;
    *mk = VisMask{nullptr, 0, 1, 1, 1.f};
    if (mask) {
        if (S < 1 || S > 46340 || Sm < 1 || Sm > 46340 || mask_bs < 1 || mask_bs > 0x7fffffffLL / (Sm * Sm)) return MODA_ESHAPE;
        *mk = VisMask{mask, (long long)mask_bs, (int)Sm, (int)S, (float)Sm / (float)S};
    }
    return 0;
}

}   // namespace

extern "C" int moda_vis_minmax(const float* x, int64_t total, const int64_t* ops, int64_t nkeys, int64_t max_n, const float* mask,
                               int64_t mask_bs, int64_t Sm, int64_t S, int32_t* part, float* mm, int32_t* status, void* stream) {
    VisMask mk;
    if (const int rc = table_shape(total, nkeys, max_n, mask, mask_bs, Sm, S, &mk)) return rc;
    if (!x || !ops || !part || !mm || !status) return MODA_EINVAL;
    const int tiles = (int)nblocks(max_n, kTile);
    hipLaunchKernelGGL(vis_minmax_tiles, dim3((unsigned)tiles, (unsigned)nkeys), dim3(kBlock), 0, (hipStream_t)stream, x, (long long)total,
                       (const VisOp*)ops, mk, tiles, (int*)part);
    hipLaunchKernelGGL(vis_minmax_keys, dim3((unsigned)nkeys), dim3(kBlock), 0, (hipStream_t)stream, (const VisOp*)ops, (long long)total, tiles,
                       (const int*)part, mm, (int*)status);
    return (int)hipGetLastError();
}

extern "C" int moda_vis_apply(const float* x, int64_t total, const int64_t* ops, int64_t nkeys, int64_t max_n, const float* mask,
                              int64_t mask_bs, int64_t Sm, int64_t S, const float* mm, float* out, void* stream) {
    VisMask mk;
    if (const int rc = table_shape(total, nkeys, max_n, mask, mask_bs, Sm, S, &mk)) return rc;
    if (!x || !ops || !mm || !out) return MODA_EINVAL;
    hipLaunchKernelGGL(vis_apply_kernel, dim3(nblocks(max_n, kTile), (unsigned)nkeys), dim3(kBlock), 0, (hipStream_t)stream, x, (long long)total,
                       (const VisOp*)ops, mk, mm, out);
    return (int)hipGetLastError();
}

extern "C" int moda_flow_color(const float* flow, int64_t N, int64_t HW, int64_t C, const float* maxrad, const float* wheel,
                               int32_t f64_after_norm, uint8_t* out, void* stream) {
    if (N < 1 || HW < 1 || N > 65535 || C < 2 || C > 65536 || HW > 0x7fffffffLL / 3 / N) return MODA_ESHAPE;
    if (!flow || !maxrad || !wheel || !out) return MODA_EINVAL;
    const dim3 grid(nblocks(HW, kBlock), (unsigned)N);
    if (f64_after_norm)
        hipLaunchKernelGGL(flow_color_kernel<double>, grid, dim3(kBlock), 0, (hipStream_t)stream, flow, (int)HW, (int)C, maxrad, wheel, out);
    else
        hipLaunchKernelGGL(flow_color_kernel<float>, grid, dim3(kBlock), 0, (hipStream_t)stream, flow, (int)HW, (int)C, maxrad, wheel, out);
    return (int)hipGetLastError();
}

extern "C" int moda_vis_grid(const float* img, int64_t N, int64_t h, int64_t w, int64_t c, int64_t row, int64_t col, float* out,
                             void* stream) {
    if (N < 1 || h < 1 || w < 1 || c < 1 || row < 1 || col < 1) return MODA_ESHAPE;
    const int64_t lim = 0x7fffffffLL;
    if (row > lim / col || N < row * col || h > lim / row || w > lim / col || c > lim / (row * h) / (col * w)) return MODA_ESHAPE;
    if (!img || !out) return MODA_EINVAL;
    const int64_t total = row * h * col * w * c;
    hipLaunchKernelGGL(vis_grid_kernel, dim3(nblocks(total, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, img, (int)h, (int)w, (int)c,
                       (int)col, (int)total, out);
    return (int)hipGetLastError();
}

extern "C" int moda_vis_to_u8(const float* frames, int64_t N, int64_t E, const int32_t* pick, int64_t P, const float* mm, uint8_t* out,
                              int32_t* status, void* stream) {
    if (N < 1 || E < 1 || P < 1 || N > 0x7fffffffLL / E || P > 0x7fffffffLL / E) return MODA_ESHAPE;
    if (!frames || !pick || !out || !status) return MODA_EINVAL;
    hipLaunchKernelGGL(vis_to_u8_kernel, dim3(nblocks(P * E, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, frames, (int)N, (int)E,
                       (const int*)pick, (long long)(P * E), mm, out, (int*)status);
    return (int)hipGetLastError();
}
