// DensePose-CSE matching (reference nnutils/geom_utils.py: ood_check_cse :1610-1663, resample_dp / bbox_dp2rnd :1665-1701,
// compute_flow_cse / match2flo / match2coords :1207-1247).  fp32 only.
//
//   feat_argmax  for every 16-channel query row the candidate row with the largest dot product; the score matrix never reaches
//                memory.  A 256-thread workgroup owns 128 queries, 32 per wave, held as the A operand of
//                v_mfma_f32_32x32x2_f32 (8 registers: k = 2 s + (lane >> 5) of step s).  Candidates pass through LDS in tiles of
//                256, stored as 16 planes (one per channel, stride 260 floats) so that the B operand of a 32-candidate column
//                block is one conflict-free 4-byte read per step.  8 chained MFMAs give 32 x 32 scores, each bit for bit the
//                fp32 chain fma(a15, b15, ... fma(a0, b0, 0)) in ascending k (one rounding per step, nothing wider inside).
//                The f32-input MFMA runs at the packed-FMA rate, but it leaves the VALU to the selection, which costs five
//                VALU operations a score -- beside 16 FMAs a score on the same pipe it would add a third to the time.
//   order        larger score wins; equal scores: the lowest candidate index; a NaN score beats every number and the lowest
//                NaN index wins (torch.argmax); -0 == +0.  A lane sees the candidates j = col (mod 32) in ascending order and
//                keeps (best, index) per query register, replacing only on !(s <= best) while best is not NaN -- so the first
//                of equals stays.  The 32 lanes of a row, and the candidate ranges of a split launch, then meet on one 64-bit
//                key: (order(score) << 32) | (0xFFFFFFFF - index), where order() maps the score's bits to an unsigned integer
//                that rises with the score (-0 first made +0, NaN = 0xFFFFFFFF).  The maximum key is the answer whatever order
//                lanes or workgroups arrive in: ranges meet in atomicMax on uint64 -- no float atomics, the same bits on every
//                run and for every split.
//   resample     one thread per destination pixel, looping over the channels; bilinear from a per-batch affine in the
//                convention of F.grid_sample (zero padding, align_corners = False) or of F.interpolate (edge clamp), optional
//                L2 normalisation over the channels (the blend is evaluated twice, not kept, so any C works).  In DP mode the
//                affine of resample_dp is composed from dp_bbox and kaug by every thread, and every workgroup repeats the
//                reference's global test dp_bbox.abs().sum() == 0 over the 4 B values: nothing is read back.
//   ood_error    per frame the mean reprojection error over the pixels with dp_idx != 0: float64 partials per thread, a
//                shuffle / LDS tree per workgroup, workgroup partials added in index order by a second kernel.  No atomics
//                except the integer count of refused dp_idx values.
// Device memory is written only by plain vector stores and HIP atomic functions.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kBlock = 256;
constexpr int kK = MODA_CSE_CHANNELS;
constexpr int kQT = MODA_CSE_QUERY_TILE;         // 4 waves x 32 queries
constexpr int kCT = MODA_CSE_CAND_TILE;          // candidates per LDS tile
constexpr int kCTP = kCT + 4;                    // plane stride: the (k, m) writes of row-major candidates hit 64 banks
constexpr int kTargetBlocks = 1024;              // four workgroups per CU on 256 CUs
constexpr int kOodMaxBlocks = MODA_OOD_MAX_BLOCKS;

DEVINL unsigned long long make_key(float s, int j) {
    unsigned u;
    if (s != s) {
        u = 0xFFFFFFFFu;
    } else {
        u = s == 0.0f ? 0u : __float_as_uint(s);                           // -0 counts as +0
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)j);
}

template <bool MASK>
DEVINL void select16(const f32x16& acc, float (&best)[16], int (&bj)[16], int j, bool ok) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float s = acc[r];
        bool upd = !(s <= best[r]) && (best[r] == best[r]);
        if (MASK) upd = upd && ok;
        best[r] = upd ? s : best[r];
        bj[r] = upd ? j : bj[r];
    }
}

// splits > 1: results go to keys through atomicMax; splits == 1: idx is written directly
__global__ __launch_bounds__(kBlock) void feat_argmax_kernel(const float* __restrict__ q, int64_t q_sb, int64_t q_sr, int64_t q_sk,
                                                            const float* __restrict__ c, int64_t c_sb, int64_t c_sr, int64_t c_sk,
                                                            int N, int M, int nqb, int splits, int range, int* __restrict__ idx,
                                                            unsigned long long* __restrict__ keys) {
    __shared__ float lds[kK * kCTP];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, col = lane & 31, h = lane >> 5;
    const int per_b = nqb * splits;
    const int b = blockIdx.x / per_b, rr = blockIdx.x - b * per_b;
    const int sp = rr / nqb, qb = rr - sp * nqb;
    const int m_begin = sp * range, m_end = min(M, m_begin + range);       // the host makes every range non-empty
    const float* qp = q + (int64_t)b * q_sb;
    const float* cp = c + (int64_t)b * c_sb;

    const int q_base = qb * kQT + w * 32;
    const int qi = min(q_base + col, N - 1);                               // lanes past N repeat the last query; not stored
    float a[kK / 2];
#pragma unroll
    for (int s = 0; s < kK / 2; ++s) a[s] = qp[(int64_t)qi * q_sr + (int64_t)(2 * s + h) * q_sk];

    float best[16];
    int bj[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        best[r] = -__builtin_inff();
        bj[r] = m_begin + col;                                             // the first candidate this lane sees, if it sees any
    }

    for (int m0 = m_begin; m0 < m_end; m0 += kCT) {
        __syncthreads();                                                   // the previous tile has been read
        const int n_here = min(kCT, m_end - m0);
        if (c_sk == 1) {                                                   // rows of 16 contiguous channels
            for (int e = t; e < kCT * kK; e += kBlock) {
                const int k = e & (kK - 1), mm = e >> 4;
                lds[k * kCTP + mm] = mm < n_here ? cp[(int64_t)(m0 + mm) * c_sr + k] : 0.0f;
            }
        } else {                                                           // channel planes (the (16, h, w) image)
            for (int e = t; e < kCT * kK; e += kBlock) {
                const int mm = e & (kCT - 1), k = e / kCT;
                lds[k * kCTP + mm] = mm < n_here ? cp[(int64_t)(m0 + mm) * c_sr + (int64_t)k * c_sk] : 0.0f;
            }
        }
        __syncthreads();
        const int nsub = (n_here + 31) >> 5;
        for (int sub = 0; sub < nsub; ++sub) {
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
            for (int s = 0; s < kK / 2; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], lds[(2 * s + h) * kCTP + sub * 32 + col], acc, 0, 0, 0);
            const int j = m0 + sub * 32 + col;
            if (m0 + sub * 32 + 32 <= m_end)
                select16<false>(acc, best, bj, j, true);
            else
                select16<true>(acc, best, bj, j, j < m_end);               // the padding of the last block never wins
        }
    }

    const bool seen = m_begin + col < m_end;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        unsigned long long key = seen ? make_key(best[r], bj[r]) : 0ull;   // a real key is never 0
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o);
            key = other > key ? other : key;
        }
        const int i = q_base + (r & 3) + 8 * (r >> 2) + 4 * h;            // the accumulator's row
        if (col == 0 && i < N) {
            const int64_t o = (int64_t)b * N + i;
            if (splits == 1)
                idx[o] = (int)(0xFFFFFFFFu - (unsigned)key);
            else
                atomicMax(&keys[o], key);
        }
    }
}

__global__ __launch_bounds__(kBlock) void argmax_unpack_kernel(const unsigned long long* __restrict__ keys, int64_t n,
                                                               int* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) idx[i] = (int)(0xFFFFFFFFu - (unsigned)keys[i]);
}

DEVINL float texel(const float* __restrict__ p, int Hs, int Ws, int y, int x) {
    return (y >= 0 && y < Hs && x >= 0 && x < Ws) ? p[(int64_t)y * Ws + x] : 0.0f;
}

struct Tap {
    int x0, y0, x1, y1;
    float wx0, wx1, wy0, wy1;
    bool any;
};

DEVINL float blend(const float* __restrict__ p, int Hs, int Ws, const Tap& tp) {
    if (!tp.any) return 0.0f;
    const float top = texel(p, Hs, Ws, tp.y0, tp.x0) * tp.wx0 + texel(p, Hs, Ws, tp.y0, tp.x1) * tp.wx1;
    const float bot = texel(p, Hs, Ws, tp.y1, tp.x0) * tp.wx0 + texel(p, Hs, Ws, tp.y1, tp.x1) * tp.wx1;
    return top * tp.wy0 + bot * tp.wy1;
}

__global__ __launch_bounds__(kBlock) void grid_resample_kernel(const float* __restrict__ src, int B, int C, int Hs, int Ws, int Hd,
                                                              int Wd, int mode, const float* __restrict__ affine,
                                                              const float* __restrict__ dp_bbox, const float* __restrict__ kaug,
                                                              int normalize, float* __restrict__ dst) {
    bool interp = mode == MODA_RESAMPLE_INTERP;
    if (mode == MODA_RESAMPLE_DP) {                                        // dp_bbox.abs().sum() == 0: every value is +-0
        int nz = 0;
        for (int i = threadIdx.x; i < 4 * B; i += kBlock) nz |= !(dp_bbox[i] == 0.0f) ? 1 : 0;
        interp = __syncthreads_or(nz) == 0;
    }
    const int64_t plane = (int64_t)Hd * Wd;
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= (int64_t)B * plane) return;
    const int b = (int)(p / plane);
    const int rem = (int)(p - (int64_t)b * plane);
    const int y = rem / Wd, x = rem - y * Wd;

    float fx, fy;
    Tap tp;
    if (interp) {
        const float sx = (float)Ws / (float)Wd, sy = (float)Hs / (float)Hd;
        fx = sx * ((float)x + 0.5f) - 0.5f;
        fy = sy * ((float)y + 0.5f) - 0.5f;
        fx = fx < 0.0f ? 0.0f : fx;
        fy = fy < 0.0f ? 0.0f : fy;
        tp.x0 = min((int)fx, Ws - 1);
        tp.y0 = min((int)fy, Hs - 1);
        tp.x1 = min(tp.x0 + 1, Ws - 1);
        tp.y1 = min(tp.y0 + 1, Hs - 1);
        tp.any = true;
    } else {
        float r00, r10, t0, r01, r11, t1;
        if (mode == MODA_RESAMPLE_DP) {
            const float* bb = dp_bbox + 4 * b;
            const float* ka = kaug + 4 * b;
            const float sx = (bb[2] - bb[0]) / 112.0f, sy = (bb[3] - bb[1]) / 112.0f;
            const float i0 = 1.0f / ka[0], i1 = 1.0f / ka[1];
            const float m00 = i0 * sx, m11 = i1 * sy;
            const float m02 = i0 * bb[0] + (-ka[2] / ka[0]), m12 = i1 * bb[1] + (-ka[3] / ka[1]);
            r00 = 1.0f / m00;
            r11 = 1.0f / m11;
            t0 = -m02 / m00;
            t1 = -m12 / m11;
            r10 = r01 = 0.0f;
        } else {
            const float* af = affine + 6 * b;
            r00 = af[0], r10 = af[1], t0 = af[2], r01 = af[3], r11 = af[4], t1 = af[5];
        }
        const float u = ((float)x * r00 + (float)y * r10) + t0;
        const float v = ((float)x * r01 + (float)y * r11) + t1;
        const float gx = u / (float)Ws * 2.0f - 1.0f, gy = v / (float)Ws * 2.0f - 1.0f;   // the reference divides both by the width
        fx = ((gx + 1.0f) * (float)Ws - 1.0f) / 2.0f;
        fy = ((gy + 1.0f) * (float)Hs - 1.0f) / 2.0f;
        tp.any = fx > -1.0f && fx < (float)Ws && fy > -1.0f && fy < (float)Hs;            // false for NaN as well
        const float flx = tp.any ? floorf(fx) : 0.0f, fly = tp.any ? floorf(fy) : 0.0f;
        tp.x0 = (int)flx;
        tp.y0 = (int)fly;
        tp.x1 = tp.x0 + 1;
        tp.y1 = tp.y0 + 1;
    }
    tp.wx1 = fx - (float)tp.x0;
    tp.wy1 = fy - (float)tp.y0;
    tp.wx0 = 1.0f - tp.wx1;
    tp.wy0 = 1.0f - tp.wy1;

    const int64_t splane = (int64_t)Hs * Ws;
    const float* sb = src + (int64_t)b * C * splane;
    float* db = dst + (int64_t)b * C * plane + rem;
    float scale = 1.0f;
    if (normalize) {
        float ss = 0.0f;
        for (int ch = 0; ch < C; ++ch) {
            const float val = blend(sb + ch * splane, Hs, Ws, tp);
            ss = ss + val * val;
        }
        scale = fmaxf(sqrtf(ss), 1e-12f);
    }
    for (int ch = 0; ch < C; ++ch) {
        const float val = blend(sb + ch * splane, Hs, Ws, tp);
        db[ch * plane] = normalize ? val / scale : val;
    }
}

__global__ __launch_bounds__(kBlock) void ood_partial_kernel(const int* __restrict__ idx, const int* __restrict__ dp_idx, int N, int h,
                                                            int w, int Hi, int Wi, int nblk, double* __restrict__ partials,
                                                            int* __restrict__ status) {
    __shared__ double lds[kBlock / 64][2];
    __shared__ int lbad[kBlock / 64];
    const int b = blockIdx.x / nblk, k = blockIdx.x - b * nblk;
    const float sy = (float)Hi / (float)h, sx = (float)Wi / (float)w;     // F.interpolate(mode='nearest'): floor(dst * (in / out))
    const int* ib = idx + (int64_t)b * N;
    const int* db = dp_idx + (int64_t)b * Hi * Wi;
    double sum = 0.0, cnt = 0.0;
    int bad = 0;
    for (int p = k * kBlock + threadIdx.x; p < h * w; p += nblk * kBlock) {
        const int y = p / w, x = p - y * w;
        const int ys = min((int)floorf((float)y * sy), Hi - 1), xs = min((int)floorf((float)x * sx), Wi - 1);
        const int d = db[(int64_t)ys * Wi + xs];
        if (d == 0) continue;
        if (d < 0 || d >= N) {                                             // never read through a bad index
            ++bad;
            continue;
        }
        const int m = ib[d];
        if (m < 0 || m >= h * w) {
            ++bad;
            continue;
        }
        const int my = m / w, mx = m - my * w;
        const float dx = (float)(mx - x), dy = (float)(my - y);
        sum += (double)sqrtf(dx * dx + dy * dy);
        cnt += 1.0;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    sum = wave_add_down(sum);
    cnt = wave_add_down(cnt);
    bad = wave_add_down(bad);
    if (lane == 0) {
        lds[wv][0] = sum;
        lds[wv][1] = cnt;
        lbad[wv] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0, n = 0.0;
        int nb = 0;
#pragma unroll
        for (int i = 0; i < kBlock / 64; ++i) {
            s += lds[i][0];
            n += lds[i][1];
            nb += lbad[i];
        }
        partials[(int64_t)blockIdx.x * 2 + 0] = s;
        partials[(int64_t)blockIdx.x * 2 + 1] = n;
        if (nb && status) atomicAdd(&status[0], nb);
    }
}

__global__ __launch_bounds__(kBlock) void ood_final_kernel(const double* __restrict__ partials, int B, int nblk, float threshold,
                                                          float* __restrict__ error, uint8_t* __restrict__ valid) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    double s = 0.0, n = 0.0;
    for (int k = 0; k < nblk; ++k) {                                       // index order: the same bits on every run
        s += partials[((int64_t)b * nblk + k) * 2 + 0];
        n += partials[((int64_t)b * nblk + k) * 2 + 1];
    }
    const float e = (float)(s / n);                                        // an empty mask: 0 / 0 = NaN, as mean() of nothing
    error[b] = e;
    valid[b] = e < threshold ? 1 : 0;
}

bool fa_shape_ok(int64_t B, int64_t N, int64_t M) {
    if (B < 1 || M < 1 || N < 0) return false;
    return (double)B * (double)N < 2147483648.0 && (double)M < 2147483648.0 - kCT;
}

void fa_plan(int64_t B, int64_t N, int64_t M, int forced, int* nqb, int* splits, int* range) {
    *nqb = (int)((N + kQT - 1) / kQT);
    const int64_t blocks = B * (int64_t)*nqb;
    const int64_t tiles = (M + kCT - 1) / kCT;
    int64_t s = forced > 0 ? forced : (blocks > 0 ? (kTargetBlocks + blocks - 1) / blocks : 1);
    s = s < 1 ? 1 : (s > tiles ? tiles : s);
    const int64_t tiles_per = (tiles + s - 1) / s;
    *range = (int)(tiles_per * kCT);
    *splits = (int)((tiles + tiles_per - 1) / tiles_per);                  // no empty range
}

int ood_blocks(int64_t hw) {
    const int64_t n = (hw + 4 * kBlock - 1) / (4 * kBlock);
    return (int)(n < 1 ? 1 : (n > kOodMaxBlocks ? kOodMaxBlocks : n));
}

}   // namespace

extern "C" int32_t moda_feat_argmax_splits(int64_t B, int64_t N, int64_t M, int32_t forced, int64_t* range) {
    if (!fa_shape_ok(B, N, M) || N == 0 || forced < 0) {
        if (range) *range = M;
        return 1;
    }
    int nqb, splits, rg;
    fa_plan(B, N, M, forced, &nqb, &splits, &rg);
    if (range) *range = rg;
    return splits;
}

extern "C" int moda_feat_argmax(const float* q, int64_t q_sb, int64_t q_sr, int64_t q_sk, const float* c, int64_t c_sb, int64_t c_sr,
                                int64_t c_sk, int64_t B, int64_t N, int64_t M, int32_t splits, int32_t* idx, uint64_t* keys,
                                void* stream) {
    if (!fa_shape_ok(B, N, M)) return MODA_ESHAPE;
    if (N == 0) return 0;
    if (!q || !c || !idx || splits < 0) return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int nqb, ns, range;
    fa_plan(B, N, M, keys ? splits : 1, &nqb, &ns, &range);                // no workspace: one range
    if ((double)B * nqb * ns >= 2147483648.0) return MODA_ESHAPE;
    if (ns > 1) {
        hipError_t e = hipMemsetAsync(keys, 0, sizeof(uint64_t) * (size_t)(B * N), st);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(feat_argmax_kernel, dim3((unsigned)(B * nqb * ns)), dim3(kBlock), 0, st, q, q_sb, q_sr, q_sk, c, c_sb, c_sr,
                       c_sk, (int)N, (int)M, nqb, ns, range, idx, (unsigned long long*)keys);
    if (ns > 1)
        hipLaunchKernelGGL(argmax_unpack_kernel, dim3(nblocks(B * N, kBlock)), dim3(kBlock), 0, st, (const unsigned long long*)keys,
                           B * N, idx);
    return (int)hipGetLastError();
}

extern "C" int moda_grid_resample(const float* src, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t Hd, int64_t Wd, int32_t mode,
                                  const float* affine, const float* dp_bbox, const float* kaug, int32_t normalize, float* dst,
                                  void* stream) {
    if (B < 1 || C < 1 || Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1) return MODA_ESHAPE;
    if ((double)B * C * Hs * Ws >= 2147483648.0 || (double)B * C * Hd * Wd >= 2147483648.0 || B >= (1 << 24)) return MODA_ESHAPE;
    if (!src || !dst) return MODA_EINVAL;
    if (mode == MODA_RESAMPLE_GRID ? !affine : mode == MODA_RESAMPLE_DP ? (!dp_bbox || !kaug) : mode != MODA_RESAMPLE_INTERP)
        return MODA_EINVAL;
    hipLaunchKernelGGL(grid_resample_kernel, dim3(nblocks(B * Hd * Wd, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, src, (int)B,
                       (int)C, (int)Hs, (int)Ws, (int)Hd, (int)Wd, mode, affine, dp_bbox, kaug, normalize, dst);
    return (int)hipGetLastError();
}

extern "C" int moda_ood_error(const int32_t* idx, const int32_t* dp_idx, int64_t B, int64_t N, int64_t h, int64_t w, int64_t Hi,
                              int64_t Wi, float threshold, double* partials, float* error, uint8_t* valid, int32_t* status,
                              void* stream) {
    if (B < 1 || N < 1 || h < 1 || w < 1 || Hi < 1 || Wi < 1) return MODA_ESHAPE;
    if ((double)B * N >= 2147483648.0 || (double)h * w >= 1073741824.0 || (double)B * Hi * Wi >= 2147483648.0) return MODA_ESHAPE;
    if (!idx || !dp_idx || !partials || !error || !valid) return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = ood_blocks(h * w);
    if ((double)B * nblk >= 2147483648.0) return MODA_ESHAPE;
    hipLaunchKernelGGL(ood_partial_kernel, dim3((unsigned)(B * nblk)), dim3(kBlock), 0, st, idx, dp_idx, (int)N, (int)h, (int)w,
                       (int)Hi, (int)Wi, nblk, partials, status);
    hipLaunchKernelGGL(ood_final_kernel, dim3(nblocks(B, kBlock)), dim3(kBlock), 0, st, (const double*)partials, (int)B, nblk,
                       threshold, error, valid);
    return (int)hipGetLastError();
}
