// Pixel sampling of a training step on the device (reference nnutils/moda.py:1048-1260, banmo.sample_pxs): the top-k of the
// uncertainty head's predictions under a total order, the per-ray assembly that replaces the reference's stack / cat loops, and
// the one-pixel-per-ray gather of the observations.  Nothing allocates, synchronises or reads back; every launch goes to the
// caller's stream.  No float atomics (the only atomics are integer counts of NaNs and refused ids), no sort: an element's rank
// under a total order is a permutation, so every output slot is written exactly once and the bits are the same on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 1024;               // composite keys of a row staged per pass (8 KiB of LDS)
constexpr int kShortN = kBlock;           // rows up to this length share a workgroup

// The order of moda_topk_rows as one unsigned compare: the high word is the value's key (-0 as +0, every NaN one key above
// +inf, otherwise the usual monotone map of the IEEE bits), the low word the complemented index, so that a LARGER composite
// comes FIRST: descending key, then ascending index.
DEVINL unsigned value_key(float v, int* is_nan) {
    unsigned b = __float_as_uint(v);
    *is_nan = (b & 0x7fffffffu) > 0x7f800000u;
    if (*is_nan) return 0xffffffffu;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
DEVINL unsigned long long composite(unsigned key, unsigned index) {
    return ((unsigned long long)key << 32) | (unsigned long long)(~index);
}

// Long rows: grid (ceil(n / kBlock), rows); every lane owns one element and counts the composites above its own while the row
// streams through LDS in tiles, each tile entry read by all lanes at one address (a broadcast).
__global__ void topk_long_kernel(const float* __restrict__ values, int n, int k, int* __restrict__ idx_out,
                                 float* __restrict__ val_out, int* __restrict__ status) {
    __shared__ unsigned long long sh[kTile];
    const long long row = blockIdx.y;
    const float* v = values + row * n;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    int nan_i = 0;
    float mine = 0.f;
    unsigned long long ci = 0;
    if (i < n) {
        mine = v[i];
        ci = composite(value_key(mine, &nan_i), (unsigned)i);
    }
    int rank = 0;
    for (int base = 0; base < n; base += kTile) {
        const int m = (n - base) < kTile ? (n - base) : kTile;
        __syncthreads();
        for (int j = threadIdx.x; j < m; j += kBlock) {
            int dummy;
            sh[j] = composite(value_key(v[base + j], &dummy), (unsigned)(base + j));
        }
        __syncthreads();
        for (int j = 0; j < m; ++j) rank += sh[j] > ci ? 1 : 0;
    }
    if (i < n) {
        if (nan_i) atomicAdd(status, 1);
        if (rank < k) {
            idx_out[row * k + rank] = i;
            if (val_out) val_out[row * k + rank] = mine;
        }
    }
}

// Short rows (n <= kShortN): a workgroup takes kBlock / n whole rows, one lane per element, the rows staged in LDS once.
__global__ void topk_short_kernel(const float* __restrict__ values, long long rows, int n, int k, int rows_per_block,
                                  int* __restrict__ idx_out, float* __restrict__ val_out, int* __restrict__ status) {
    __shared__ unsigned long long sh[kBlock];
    const int lr = threadIdx.x / n;                    // local row
    const int i = threadIdx.x - lr * n;
    const long long row = (long long)blockIdx.x * rows_per_block + lr;
    const bool live = lr < rows_per_block && row < rows;
    int nan_i = 0;
    float mine = 0.f;
    unsigned long long ci = 0;
    if (live) {
        mine = values[row * n + i];
        ci = composite(value_key(mine, &nan_i), (unsigned)i);
        sh[threadIdx.x] = ci;                          // threadIdx.x == lr * n + i
    }
    __syncthreads();
    if (!live) return;
    const unsigned long long* r = sh + lr * n;
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += r[j] > ci ? 1 : 0;
    if (nan_i) atomicAdd(status, 1);
    if (rank < k) {
        idx_out[row * k + rank] = i;
        if (val_out) val_out[row * k + rank] = mine;
    }
}

struct AsmArgs {
    const long long* rand_inds;      // (bs, 5 nsample)
    const void *lineid, *frameid, *frameid_sub, *dataid, *errid;
    const int* topk;                 // line mode (K,), frame mode (bs, n_s); unused when n_s == 0
    const float* near_far;           // (n_frames, 2)
    long long bs, img_size, n_frames, n_vid;
    int nsample, n_u, n_s, line_mode, ids64;
    long long *rand_out, *frameid_out, *frameid_sub_out, *dataid_out, *errid_out, *batch_map_out;
    float *xys_out, *near_far_out;
    int* status;
};

// One thread per output ray.  Line mode (lines b = h P + l): half h owns rays h (P n_u + K) + ..., first the P n_u uniform rays
// (l, j < n_u) at column rand_inds[b, j], then the K = n_s P active rays t with candidate c = topk[t], l = c / (4 nsample),
// j = c % (4 nsample), column rand_inds[b, nsample + j]; the same c serves both halves (moda.py:1149-1158).  Frame mode: ray
// (b, s) reads rand_inds[b, s] for s < n_u and rand_inds[b, nsample + topk[b, s - n_u]] after; the per-frame entries are
// written by the frame's first ray.
__global__ void pxs_assemble_kernel(AsmArgs a, long long R) {
    const long long r = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (r >= R) return;
    const long long stride = 5LL * a.nsample, n_a = 4LL * a.nsample;
    const float nan = __uint_as_float(0x7fc00000u);
    long long b, slot;                // the line / frame the ray comes from and its entry of rand_inds[b]
    bool slot_ok = true;
    if (a.line_mode) {
        const long long P = a.bs / 2, K = (long long)a.n_s * P, half = P * a.n_u + K;
        const long long h = r / half, q = r - h * half;
        long long l;
        if (q < P * a.n_u) {
            l = q / a.n_u;
            slot = q - l * a.n_u;
        } else {
            const long long c = a.topk[q - P * a.n_u];
            slot_ok = c >= 0 && c < P * n_a;
            l = slot_ok ? c / n_a : 0;
            slot = a.nsample + (slot_ok ? c - l * n_a : 0);
        }
        b = h * P + l;
    } else {
        const long long per = a.n_u + a.n_s;
        b = r / per;
        const long long s = r - b * per;
        if (s < a.n_u) {
            slot = s;
        } else {
            const long long c = a.topk[b * a.n_s + (s - a.n_u)];
            slot_ok = c >= 0 && c < n_a;
            slot = a.nsample + (slot_ok ? c : 0);
        }
    }
    const long long ind = a.rand_inds[b * stride + slot];
    const long long limit = a.line_mode ? a.img_size : a.img_size * a.img_size;
    const bool col_ok = slot_ok && ind >= 0 && ind < limit;
    a.rand_out[r] = slot_ok ? ind : -1;
    float x = nan, y = nan;
    if (col_ok) {
        if (a.line_mode) {
            x = (float)ind;
            y = (float)load_id(a.lineid, a.ids64, b);
        } else {
            const long long yy = ind / a.img_size;
            x = (float)(ind - yy * a.img_size);
            y = (float)yy;
        }
    } else {
        atomicAdd(a.status + 2, 1);
    }
    a.xys_out[r * 2] = x;
    a.xys_out[r * 2 + 1] = y;
    long long o;                      // where the per-ray (line mode) / per-frame (frame mode) entries go
    if (a.line_mode) {
        o = r;
    } else {
        if (r != b * (a.n_u + a.n_s)) return;
        o = b;
    }
    const long long f = load_id(a.frameid, a.ids64, b), d = load_id(a.dataid, a.ids64, b);
    a.frameid_out[o] = f;
    a.frameid_sub_out[o] = load_id(a.frameid_sub, a.ids64, b);
    a.dataid_out[o] = d;
    a.errid_out[o] = load_id(a.errid, a.ids64, b);
    a.batch_map_out[o] = b;
    const bool f_ok = f >= 0 && f < a.n_frames;
    a.near_far_out[o * 2] = f_ok ? a.near_far[f * 2] : nan;
    a.near_far_out[o * 2 + 1] = f_ok ? a.near_far[f * 2 + 1] : nan;
    int bad = f_ok ? 0 : 1;
    if (a.n_vid > 0 && (d < 0 || d >= a.n_vid)) ++bad;
    if (bad) atomicAdd(a.status + 1, bad);
}

constexpr int kObsChannels = 24;      // img 3 | sil 1 | vis 1 | flo 2 | cfd 1 | feats 16

// One thread per (ray, channel): out[r, c] = t[row, c, col] with row = batch_map[r] (or r / ns without a map) and
// col = cols[r].  A row outside [0, B) or a column outside [0, W) is never followed: the ray's channels are NaN.
__global__ void obs_gather_kernel(const float* __restrict__ imgs, const float* __restrict__ masks, const float* __restrict__ vis2d,
                                  const float* __restrict__ flow, const float* __restrict__ occ, const float* __restrict__ feats,
                                  long long B, long long W, const long long* __restrict__ batch_map,
                                  const long long* __restrict__ cols, long long R, long long ns, int channels,
                                  float* __restrict__ img_o, float* __restrict__ sil_o, float* __restrict__ vis_o,
                                  float* __restrict__ flo_o, float* __restrict__ cfd_o, float* __restrict__ feat_o,
                                  int* __restrict__ status) {
    const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= R * channels) return;
    const long long r = t / channels;
    const int ch = (int)(t - r * channels);
    const long long row = batch_map ? batch_map[r] : r / ns, col = cols[r];
    const bool row_ok = row >= 0 && row < B, col_ok = col >= 0 && col < W;
    if (status && ch == 0) {
        if (!row_ok) atomicAdd(status + 1, 1);
        if (!col_ok) atomicAdd(status + 2, 1);
    }
    const float* src;
    float* dst;
    int C, c;
    if (ch < 3) { src = imgs; dst = img_o; C = 3; c = ch; }
    else if (ch < 4) { src = masks; dst = sil_o; C = 1; c = 0; }
    else if (ch < 5) { src = vis2d; dst = vis_o; C = 1; c = 0; }
    else if (ch < 7) { src = flow; dst = flo_o; C = 2; c = ch - 5; }
    else if (ch < 8) { src = occ; dst = cfd_o; C = 1; c = 0; }
    else { src = feats; dst = feat_o; C = 16; c = ch - 8; }
    dst[r * C + c] = (row_ok && col_ok) ? src[(row * C + c) * W + col] : __uint_as_float(0x7fc00000u);
}

}   // namespace

extern "C" int moda_topk_rows(const float* values, int64_t rows, int64_t n, int64_t k, int32_t* idx_out, float* val_out,
                              int32_t* status, void* stream) {
    if (rows < 0 || n < 1 || n > MODA_TOPK_MAX_N || rows > 0x7fffffffLL / n || (n > kShortN && rows > 65535)) return MODA_ESHAPE;
    if (k < 1 || k > n) return MODA_EINVAL;
    if (rows == 0) return 0;
    if (!values || !idx_out || !status) return MODA_EINVAL;
    if (n <= kShortN) {
        const int rpb = kBlock / (int)n;
        hipLaunchKernelGGL(topk_short_kernel, dim3(nblocks(rows, rpb)), dim3(kBlock), 0, (hipStream_t)stream, values, (long long)rows,
                           (int)n, (int)k, rpb, (int*)idx_out, val_out, (int*)status);
    } else {
        hipLaunchKernelGGL(topk_long_kernel, dim3(nblocks(n, kBlock), (unsigned)rows), dim3(kBlock), 0, (hipStream_t)stream, values,
                           (int)n, (int)k, (int*)idx_out, val_out, (int*)status);
    }
    return (int)hipGetLastError();
}

extern "C" int moda_pxs_assemble(const int64_t* rand_inds, int64_t bs, int32_t nsample, int32_t n_u, int32_t n_s, int32_t line_mode,
                                 int64_t img_size, const void* lineid, const void* frameid, const void* frameid_sub,
                                 const void* dataid, const void* errid, int32_t ids64, const int32_t* topk, const float* near_far,
                                 int64_t n_frames, int64_t n_vid, int64_t* rand_out, float* xys_out, int64_t* frameid_out,
                                 int64_t* frameid_sub_out, int64_t* dataid_out, int64_t* errid_out, int64_t* batch_map_out,
                                 float* near_far_out, int32_t* status, void* stream) {
    if (bs < 1 || nsample < 1 || n_u < 0 || n_s < 0 || n_u + n_s < 1 || n_u > nsample || n_s > 4 * nsample || img_size < 1 ||
        img_size > 32768 || n_frames < 1 || n_vid < 0 || (line_mode && bs % 2))
        return MODA_EINVAL;
    const long long per = (long long)n_u + n_s;
    if (bs > 0x7fffffffLL / (5LL * nsample)) return MODA_ESHAPE;
    if (!rand_inds || !frameid || !frameid_sub || !dataid || !errid || !near_far || (line_mode && !lineid) || (n_s > 0 && !topk) ||
        !rand_out || !xys_out || !frameid_out || !frameid_sub_out || !dataid_out || !errid_out || !batch_map_out || !near_far_out ||
        !status)
        return MODA_EINVAL;
    AsmArgs a;
    a.rand_inds = (const long long*)rand_inds;
    a.lineid = lineid; a.frameid = frameid; a.frameid_sub = frameid_sub; a.dataid = dataid; a.errid = errid;
    a.topk = (const int*)topk; a.near_far = near_far;
    a.bs = bs; a.img_size = img_size; a.n_frames = n_frames; a.n_vid = n_vid;
    a.nsample = nsample; a.n_u = n_u; a.n_s = n_s; a.line_mode = line_mode ? 1 : 0; a.ids64 = ids64 ? 1 : 0;
    a.rand_out = (long long*)rand_out; a.frameid_out = (long long*)frameid_out; a.frameid_sub_out = (long long*)frameid_sub_out;
    a.dataid_out = (long long*)dataid_out; a.errid_out = (long long*)errid_out; a.batch_map_out = (long long*)batch_map_out;
    a.xys_out = xys_out; a.near_far_out = near_far_out; a.status = (int*)status;
    const long long R = bs * per;
    hipLaunchKernelGGL(pxs_assemble_kernel, dim3(nblocks(R, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, a, R);
    return (int)hipGetLastError();
}

extern "C" int moda_obs_gather(const float* imgs, const float* masks, const float* vis2d, const float* flow, const float* occ,
                               const float* dp_feats, int64_t B, int64_t W, const int64_t* batch_map, const int64_t* cols, int64_t R,
                               int64_t ns, float* img_at, float* sil_at, float* vis_at, float* flo_at, float* cfd_at, float* feats_at,
                               int32_t* status, void* stream) {
    if (R == 0) return 0;
    if (B < 1 || W < 1 || R < 0 || ns < 1 || B > 0x7fffffffLL || W > 0x7fffffffLL || R > 0x7fffffffLL) return MODA_ESHAPE;
    if (!imgs || !masks || !vis2d || !flow || !occ || !cols || !img_at || !sil_at || !vis_at || !flo_at || !cfd_at ||
        (dp_feats && !feats_at) || (!batch_map && (R % ns || R / ns > B)))
        return MODA_EINVAL;
    const int channels = dp_feats ? kObsChannels : 8;
    hipLaunchKernelGGL(obs_gather_kernel, dim3(nblocks(R * channels, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, imgs, masks, vis2d,
                       flow, occ, dp_feats, (long long)B, (long long)W, (const long long*)batch_map, (const long long*)cols,
                       (long long)R, (long long)ns, channels, img_at, sil_at, vis_at, flo_at, cfd_at, feats_at, (int*)status);
    return (int)hipGetLastError();
}
