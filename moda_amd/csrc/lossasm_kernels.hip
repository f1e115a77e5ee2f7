// The stage of the reference's training step between render_rays and backward() with the flags the reference trains with
// (nnutils/moda.py:164-168 root_sm, loss_flt, rm_novp all True), device-resident: no host synchronisation, no allocation, every
// launch on the caller's stream, so the whole stage can be captured into the step's graph.
//
//   loss filter, line mode   (nnutils/loss_utils.py:432-445 loss_filter_line)  three launches:
//       claim   one thread per ray: owner[errid] = max(owner[errid], ray) -- an INTEGER atomic, whose result does not depend on the
//               order the rays arrive in: the highest ray index wins a slot, as numpy's fancy assignment leaves it.
//       rows    one wavefront per frame: every slot of the frame's row takes its owner's value (and gives the owner word back as
//               -1, the state `owner` is in between calls), the row's sum is formed in float64 -- lane l adds the slots l, l + 64,
//               ... in order, the lanes are joined by the xor butterfly 32..1 (wave_add) -- and mean = sum / (1e-9 + #positive).
//       final   one workgroup: the median of the positive means by exact ranking (ties broken by the frame index), the frames'
//               flags mean > median * scale_factor in float64, invalid[i] = flag[frameid[i]] and the status counters.
//   loss filter, frame mode  (:447-476 loss_filter + the state update of moda.py:533)  one launch of one workgroup.
//   root smoothness          (:486-517 compute_root_sm_2nd_loss, geom_utils.py:1196-1205 rot_angle)  one workgroup forward (the pose
//               helpers and block_sums of pose_loss.h, shared with the first-order loss of warmup_kernels.hip); the
//               backward is a gather: one thread per frame sums the up to three triples the frame belongs to, in a fixed order.
//   loss assembly            (moda.py:517-768)  total <- carry_t * total + weight_t * mean_t over the terms in order, times total_wt:
//               one wavefront per term forward, one launch backward.  loss_utils.total_loss (no scale / drop / carry) and
//               masked_mean (one term of weight 1) are calls of the same entry.
// No float atomics anywhere: for given inputs every sum has one fixed tree.  Device memory is written by plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "moda_dev.h"
#include "pose_loss.h"

#pragma clang fp contract(off)

namespace {

// ---- loss filter ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void flt_claim_kernel(const void* __restrict__ errid, int e64, int N, long long slots,
                                                        int* __restrict__ owner) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const long long id = load_id(errid, e64, i);
    if (id < 0 || id >= slots) return;
    atomicMax(&owner[id], i);
}

__global__ __launch_bounds__(256) void flt_rows_kernel(const float* __restrict__ v, float* __restrict__ sil_err, int* __restrict__ owner,
                                                       int N, int T, int S, double* __restrict__ mean) {
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (f >= T) return;
    double s = 0.0;
    int c = 0;
    for (int j = lane; j < S; j += 64) {
        const long long slot = (long long)f * S + j;
        const int o = owner[slot];
        float x;
        if (o >= 0 && o < N) {
            x = v[o];
            sil_err[slot] = x;
        } else {
            x = sil_err[slot];
        }
        if (o != -1) owner[slot] = -1;
        s += (double)x;
        c += x > 0.f ? 1 : 0;
    }
    s = wave_add(s);
    c = wave_add(c);
    if (lane == 0) mean[f] = s / (1e-9 + (double)c);
}

// numpy's median of the positive entries of v(0..T): K of them; entry f has rank #{g: v_g < v_f, or v_g == v_f and g < f}; the
// entries of rank (K - 1) / 2 and K / 2 are averaged (one entry twice when K is odd: (a + a) / 2 = a).  K == 0: NaN.
// Every thread of the workgroup calls it.  The values are staged once in LDS (sh_v, T <= kMaxFrames doubles), so the
// O(T^2 / blockDim) comparisons per thread read LDS at a wave-uniform address (a broadcast), not global memory.
constexpr int kMaxFrames = 8000;                                    // 64000 bytes of the 64 KB a workgroup may declare

template <class Load>
DEVINL double median_positive(const Load& v, int T, double* sh_v, int* sh_k, double* sh_med) {
    if (threadIdx.x == 0) *sh_k = 0;
    int mine = 0;
    for (int f = threadIdx.x; f < T; f += blockDim.x) {
        const double m = v(f);
        sh_v[f] = m;
        mine += m > 0.0 ? 1 : 0;
    }
    __syncthreads();
    if (mine) atomicAdd(sh_k, mine);
    __syncthreads();
    const int K = *sh_k;
    for (int f = threadIdx.x; f < T; f += blockDim.x) {
        const double m = sh_v[f];
        if (!(m > 0.0)) continue;
        int rank = 0;
        for (int g = 0; g < T; ++g) {
            const double mg = sh_v[g];
            rank += (mg > 0.0 && (mg < m || (mg == m && g < f))) ? 1 : 0;
        }
        if (rank == (K - 1) / 2) sh_med[0] = m;
        if (rank == K / 2) sh_med[1] = m;
    }
    __syncthreads();
    return K > 0 ? (sh_med[0] + sh_med[1]) / 2.0 : __longlong_as_double(0x7ff8000000000000LL);
}

__global__ __launch_bounds__(1024) void flt_final_kernel(const double* __restrict__ mean, int T, double scale,
                                                         const void* __restrict__ frameid, int f64, const void* __restrict__ errid,
                                                         int e64, int N, long long slots, uint8_t* __restrict__ flag,
                                                         uint8_t* __restrict__ invalid, int* __restrict__ status) {
    __shared__ int sh_k, sh_cnt[2];
    __shared__ double sh_med[2], sh_v[kMaxFrames];
    if (threadIdx.x == 0) { sh_cnt[0] = 0; sh_cnt[1] = 0; }
    const double med = median_positive([&](int f) { return mean[f]; }, T, sh_v, &sh_k, sh_med);
    const double thr = med * scale;
    for (int f = threadIdx.x; f < T; f += blockDim.x) flag[f] = mean[f] > thr ? 1 : 0;      // NaN on either side: not flagged
    __syncthreads();
    int oob = 0, ninv = 0;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const long long eid = load_id(errid, e64, i), fid = load_id(frameid, f64, i);
        oob += (eid < 0 || eid >= slots) ? 1 : 0;
        uint8_t inv = 0;
        if (fid < 0 || fid >= T) oob += 1;
        else inv = flag[fid];
        invalid[i] = inv;
        ninv += inv;
    }
    if (oob) atomicAdd(&sh_cnt[0], oob);
    if (ninv) atomicAdd(&sh_cnt[1], ninv);
    __syncthreads();
    if (threadIdx.x == 0) { status[0] = sh_cnt[0]; status[1] = sh_cnt[1]; status[2] = sh_k; status[3] = 0; }
}

// frame mode: x (bs, n) values, m (bs, n) mask (float, or uint8 / bool when m_u8), state (T) the per-frame history.
__global__ __launch_bounds__(1024) void flt_frame_kernel(const float* __restrict__ x, const void* __restrict__ m, int m_u8, int bs,
                                                         long long n, float* __restrict__ state, int T, const void* __restrict__ errid,
                                                         int e64, double scale, float* __restrict__ flo_err,
                                                         uint8_t* __restrict__ invalid, int* __restrict__ status) {
    __shared__ int sh_k, sh_cnt[2];
    __shared__ double sh_med[2], sh_v[kMaxFrames];
    if (threadIdx.x == 0) { sh_cnt[0] = 0; sh_cnt[1] = 0; }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    for (int b = wave; b < bs; b += waves) {                     // (x * m).sum(1) / (1e-9 + m.sum(1)), the sums in float64
        double s = 0.0, ms = 0.0;
        for (long long j = lane; j < n; j += 64) {
            const long long e = (long long)b * n + j;
            const float mf = m_u8 ? (((const uint8_t*)m)[e] ? 1.f : 0.f) : ((const float*)m)[e];
            s += (double)(x[e] * mf);
            ms += (double)mf;
        }
        s = wave_add(s);
        ms = wave_add(ms);
        if (lane == 0) flo_err[b] = (float)s / (1e-9f + (float)ms);
    }
    // the median of the history BEFORE this step's update (median_positive's barriers also publish flo_err to the workgroup)
    const double med = median_positive([&](int f) { return (double)state[f]; }, T, sh_v, &sh_k, sh_med);
    const double thr = med * scale;
    int oob = 0, ninv = 0;
    for (int b = threadIdx.x; b < bs; b += blockDim.x) {
        const uint8_t inv = (double)flo_err[b] > thr ? 1 : 0;
        invalid[b] = inv;
        ninv += inv;
    }
    __syncthreads();                                              // every read of the old history lies before this line
    for (int b = threadIdx.x; b < bs; b += blockDim.x) {          // state[errid] = flo_err: the highest row wins a repeated id
        const long long id = load_id(errid, e64, b);
        if (id < 0 || id >= T) { oob += 1; continue; }
        bool last = true;
        for (int b2 = b + 1; b2 < bs; ++b2) last = last && load_id(errid, e64, b2) != id;
        if (last) state[id] = flo_err[b];
    }
    if (oob) atomicAdd(&sh_cnt[0], oob);
    if (ninv) atomicAdd(&sh_cnt[1], ninv);
    __syncthreads();
    if (threadIdx.x == 0) { status[0] = sh_cnt[0]; status[1] = sh_cnt[1]; status[2] = sh_k; status[3] = 0; }
}

// ---- root smoothness -----------------------------------------------------------------------------------------------------
// C = X Y^T, each entry the products k = 0, 1, 2 added in that order
DEVINL void mul_abt(const float X[9], const float Y[9], float C[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) C[3 * i + k] = X[3 * i] * Y[3 * k] + X[3 * i + 1] * Y[3 * k + 1] + X[3 * i + 2] * Y[3 * k + 2];
}

struct Triple {
    float R0[9], R1[9], R2[9], A[9], B[9], d[3];
    float cosv, trn;
};

DEVINL void triple_eval(const float* __restrict__ rtk, int stride, long long j, Triple& q) {
    float t0[3], t1[3], t2[3];
    load_pose(rtk, stride, j, q.R0, t0);
    load_pose(rtk, stride, j + 1, q.R1, t1);
    load_pose(rtk, stride, j + 2, q.R2, t2);
    mul_abt(q.R0, q.R1, q.A);                                     // rot_sub1 = R0 R1^T
    mul_abt(q.R1, q.R2, q.B);                                     // rot_sub2 = R1 R2^T
    q.cosv = cos_of(q.A, q.B);                                    // from the trace of rot_sub1 rot_sub2^T
#pragma unroll
    for (int c = 0; c < 3; ++c) q.d[c] = (t0[c] - t1[c]) - (t1[c] - t2[c]);
    q.trn = sqrtf(q.d[0] * q.d[0] + q.d[1] * q.d[1] + q.d[2] * q.d[2]);
}

// out[0] = loss, out[1] = 0.1 * mean(angle), out[2] = mean(trn), out[3] = #triples
__global__ __launch_bounds__(1024) void root_sm_fwd_kernel(const float* __restrict__ rtk, int stride, int T, const int* __restrict__ off,
                                                           int V, float* __restrict__ out) {
    __shared__ double sh_a[16], sh_t[16];
    __shared__ int sh_c[16];
    double sa = 0.0, st = 0.0;
    int cnt = 0;
    for (int j = threadIdx.x; j < T; j += blockDim.x) {           // j: the first frame of a triple
        int start, end;
        if (!video_of(off, V, T, j, start, end) || j + 2 >= end) continue;
        Triple q;
        triple_eval(rtk, stride, j, q);
        sa += (double)angle_of(q.cosv);
        st += (double)q.trn;
        cnt += 1;
    }
    block_sums<16>(sa, st, cnt, sh_a, sh_t, sh_c);
    if (threadIdx.x == 0) {
        const float rot = (float)(sa / (double)cnt) * 1e-1f;      // no triple: 0 / 0 = NaN, the mean of an empty set
        const float trn = (float)(st / (double)cnt);
        out[0] = (rot + trn) * 0.1f;
        out[1] = rot;
        out[2] = trn;
        out[3] = (float)cnt;
    }
}

__global__ __launch_bounds__(256) void root_sm_bwd_kernel(const float* __restrict__ rtk, int stride, int T, const int* __restrict__ off,
                                                          int V, const float* __restrict__ out, const float* __restrict__ g,
                                                          float* __restrict__ drtk) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= T) return;
    float dR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dt[3] = {0.f, 0.f, 0.f};
    int start, end;
    if (video_of(off, V, T, f, start, end)) {
        const float cnt = out[3];
        const float ca = g[0] * 0.1f * 1e-1f / cnt, ct = g[0] * 0.1f / cnt;
        for (int r = 0; r < 3; ++r) {                              // frame f as the first, middle, last frame of a triple
            const int j = f - r;
            if (j < start || j + 2 >= end) continue;
            Triple q;
            triple_eval(rtk, stride, j, q);
            // acos'(c) = -1 / sqrt(1 - c^2) where the cosine is not clamped (torch passes the gradient AT the bounds), times 1/2;
            // -ca / sqrt(..) rounds differently from ca * dangle_of(c): this kernel keeps its own form
            const float gc = (q.cosv >= kCosLo && q.cosv <= kCosHi) ? -ca / sqrtf(1.f - q.cosv * q.cosv) * 0.5f : 0.f;
            const float gt = q.trn > 0.f ? ct / q.trn : 0.f;       // torch's norm backward: 0 at norm 0
            const float sgn = r == 1 ? -2.f : 1.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) dt[c] += sgn * gt * q.d[c];
            // cos = <A, B> / 2 - 1/2: dA = gc B, dB = gc A;  A = R0 R1^T, B = R1 R2^T
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    float s = 0.f;
                    if (r == 0) {                                  // dR0 = dA R1
                        for (int k = 0; k < 3; ++k) s += q.B[3 * a + k] * q.R1[3 * k + b];
                    } else if (r == 1) {                           // dR1 = dA^T R0 + dB R2
                        for (int k = 0; k < 3; ++k) s += q.B[3 * k + a] * q.R0[3 * k + b];
                        for (int k = 0; k < 3; ++k) s += q.A[3 * a + k] * q.R2[3 * k + b];
                    } else {                                       // dR2 = dB^T R1
                        for (int k = 0; k < 3; ++k) s += q.A[3 * k + a] * q.R1[3 * k + b];
                    }
                    dR[3 * a + b] += gc * s;
                }
        }
    }
    store_pose_grad(drtk, stride, f, dR, dt);
}

// ---- loss assembly -------------------------------------------------------------------------------------------------------
constexpr int kMaxTerms = 16;
struct AsmTerms { moda_asm_term t[kMaxTerms]; int n; float total_wt; };

DEVINL bool asm_row_selected(const moda_asm_term& q, long long i) {
    if (q.mask_kind == 1) return ((const float*)q.mask)[i] > 0.f;
    if (q.mask_kind == 2) return ((const unsigned char*)q.mask)[i] != 0;
    if (q.mask_kind == 3) return ((const float*)q.mask)[i] != 0.f;
    return true;
}

// sums of one term over the rows lane, lane + 64, ...: eight rows per lane in flight.  The map and the order of every sum are
// pinned bit for bit by tests/golden/g31_total_loss_bits.npz (recorded from the kernel this one replaced): keep both.
template <int MK, bool K1, bool SD>
DEVINL void asm_term_sums(const moda_asm_term& q, int lane, float& sx, float& sm) {
    for (long long base = 0; base < q.n; base += 64 * 8) {
        float xs[8], ms[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const long long i = base + u * 64 + lane;
            const bool ok = i < q.n;
            const long long ii = ok ? i : 0;                       // (clamped: every load is unconditional and in bounds)
            bool sel = ok;
            if (MK == 1) { const float mv = ((const float*)q.mask)[ii]; sel = ok & (mv > 0.f); }
            if (MK == 2) { const unsigned char mv = ((const unsigned char*)q.mask)[ii]; sel = ok & (mv != 0); }
            if (MK == 3) { const float mv = ((const float*)q.mask)[ii]; sel = ok & (mv != 0.f); }
            ms[u] = sel ? 1.f : 0.f;
            float sc = 1.f, keep = 1.f;
            if (SD) {
                if (q.scale) sc = q.scale[ii];
                if (q.drop) keep = q.drop[ii] ? 0.f : 1.f;
            }
            if (K1) {
                xs[u] = SD ? (q.x[ii] * keep) * sc : q.x[ii];      // products, as the reference's `*= 0`: NaN * 0 stays NaN
            } else {
                float r = 0.f;
                for (int c = 0; c < q.k; ++c) r += SD ? (q.x[ii * q.k + c] * keep) * sc : q.x[ii * q.k + c];
                xs[u] = r;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            sm += ms[u];
            sx += ms[u] != 0.f ? xs[u] : 0.f;
        }
    }
}

template <bool SD>
DEVINL void asm_term_dispatch(const moda_asm_term& q, int lane, float& sx, float& sm) {
    // the mask kind and k == 1 are chosen ONCE, outside the row loop: with the tests inside it every load sat behind a branch
    // and the wave waited for each of them in turn (27 us for 8 x 2048 rows)
    switch (q.mask_kind * 2 + (q.k == 1 ? 1 : 0)) {
        case 0: asm_term_sums<0, false, SD>(q, lane, sx, sm); break;
        case 1: asm_term_sums<0, true, SD>(q, lane, sx, sm); break;
        case 2: asm_term_sums<1, false, SD>(q, lane, sx, sm); break;
        case 3: asm_term_sums<1, true, SD>(q, lane, sx, sm); break;
        case 4: asm_term_sums<2, false, SD>(q, lane, sx, sm); break;
        case 5: asm_term_sums<2, true, SD>(q, lane, sx, sm); break;
        case 6: asm_term_sums<3, false, SD>(q, lane, sx, sm); break;
        default: asm_term_sums<3, true, SD>(q, lane, sx, sm); break;
    }
}

// out[0] = total, out[1 + t] = weight_t * mean_t, out[1 + T + t] = den_t = k_t * #selected, out[1 + 2 T + t] = mean_t
__global__ __launch_bounds__(1024) void loss_asm_fwd_kernel(AsmTerms a, float* __restrict__ out) {
    __shared__ float term_s[kMaxTerms];
    // (readfirstlane: the wave index is uniform, so the term is fetched with scalar loads from the kernel arguments; indexed by
    //  a per-lane value the compiler would copy all sixteen terms to scratch first -- 20-30 us of dispatch + spill for this kernel)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (wave < a.n) {                       // one wavefront per term (16 waves, <= 16 terms): the terms are summed concurrently
        const moda_asm_term q = a.t[wave];
        float sx = 0.f, sm = 0.f;
        if (q.scale || q.drop) asm_term_dispatch<true>(q, lane, sx, sm);
        else asm_term_dispatch<false>(q, lane, sx, sm);
        const float tx = comp_wave_sum(sx), tm = comp_wave_sum(sm);
        const float den = tm * (float)q.k;
        const float mean = tx / den;                               // nothing selected: 0 / 0 = NaN
        const float term = q.weight * mean;
        if (lane == 0) { term_s[wave] = term; out[1 + wave] = term; out[1 + a.n + wave] = den; out[1 + 2 * a.n + wave] = mean; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float total = 0.f;
        for (int t = 0; t < a.n; ++t) total = a.t[t].carry * total + term_s[t];     // carry 0 is `total * 0.`: a NaN carries
        out[0] = total * a.total_wt;
    }
}

__global__ __launch_bounds__(256) void loss_asm_bwd_kernel(AsmTerms a, const float* __restrict__ out, const float* __restrict__ g) {
    const int t = blockIdx.y;
    const moda_asm_term q = a.t[t];
    if (!q.dx) return;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= q.n * q.k) return;
    const long long row = e / q.k;
    float c = g[0] * a.total_wt;
    c = c * q.weight;
    for (int s = t + 1; s < a.n; ++s) c = c * a.t[s].carry;
    c = c / out[1 + a.n + t];
    if (q.scale) c = c * q.scale[row];
    if (q.drop) c = c * (q.drop[row] ? 0.f : 1.f);
    q.dx[e] = asm_row_selected(q, row) ? c : 0.f;
}

}  // namespace

extern "C" int64_t moda_loss_filter_ws_bytes(int64_t num_frames, int64_t img_size) {
    if (num_frames < 1 || img_size < 1) return 0;
    return 8 * num_frames + 4 * num_frames * img_size + ((num_frames + 7) / 8) * 8;
}

extern "C" int moda_loss_filter_line(const float* values, const void* errid, int32_t errid64, const void* frameid, int32_t frameid64,
                                     int64_t N, float* sil_err, int64_t num_frames, int64_t img_size, double scale_factor, void* ws,
                                     uint8_t* invalid, int32_t* status, void* stream) {
    if (!values || !errid || !frameid || !sil_err || !ws || !invalid || !status) return MODA_EINVAL;
    if (N < 1 || N >= (1LL << 31) || num_frames < 1 || num_frames > kMaxFrames || img_size < 1 || num_frames * img_size >= (1LL << 31))
        return MODA_EINVAL;
    if ((uintptr_t)ws & 7) return MODA_EINVAL;
    const long long slots = num_frames * img_size;
    double* mean = (double*)ws;                                   // layout of moda_loss_filter_ws_bytes
    int* owner = (int*)(mean + num_frames);
    uint8_t* flag = (uint8_t*)(owner + slots);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(flt_claim_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, errid, (int)errid64, (int)N, slots, owner);
    hipLaunchKernelGGL(flt_rows_kernel, dim3((unsigned)((num_frames + 3) / 4)), dim3(256), 0, st, values, sil_err, owner, (int)N,
                       (int)num_frames, (int)img_size, mean);
    hipLaunchKernelGGL(flt_final_kernel, dim3(1), dim3(1024), 0, st, (const double*)mean, (int)num_frames, scale_factor, frameid,
                       (int)frameid64, errid, (int)errid64, (int)N, slots, flag, invalid, status);
    return (int)hipGetLastError();
}

extern "C" int moda_loss_filter_frame(const float* x, const void* mask, int32_t mask_u8, int64_t bs, int64_t n, float* state,
                                      int64_t num_frames, const void* errid, int32_t errid64, double scale_factor, float* flo_err,
                                      uint8_t* invalid, int32_t* status, void* stream) {
    if (!x || !mask || !state || !errid || !flo_err || !invalid || !status) return MODA_EINVAL;
    if (bs < 1 || bs > 4096 || n < 1 || bs * n >= (1LL << 31) || num_frames < 1 || num_frames > kMaxFrames) return MODA_EINVAL;
    hipLaunchKernelGGL(flt_frame_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, x, mask, (int)mask_u8, (int)bs, (long long)n, state,
                       (int)num_frames, errid, (int)errid64, scale_factor, flo_err, invalid, status);
    return (int)hipGetLastError();
}

extern "C" int moda_root_sm(const float* rtk, int32_t rows, int64_t T, const int32_t* offsets, int32_t n_videos, float* out4,
                            const float* g, float* drtk, void* stream) {
    if (!pose_args_ok(rtk, rows, T) || !offsets || !out4 || n_videos < 1 || !al16(drtk)) return MODA_EINVAL;
    const int stride = rows * 4;
    if (g) {
        if (!drtk) return MODA_EINVAL;
        hipLaunchKernelGGL(root_sm_bwd_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rtk, stride, (int)T,
                           offsets, (int)n_videos, (const float*)out4, g, drtk);
    } else {
        hipLaunchKernelGGL(root_sm_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rtk, stride, (int)T, offsets, (int)n_videos,
                           out4);
    }
    return (int)hipGetLastError();
}

extern "C" int moda_loss_assembly(const moda_asm_term* terms, int32_t n_terms, float total_wt, float* out, const float* g,
                                  void* stream) {
    if (!terms || n_terms < 1 || n_terms > kMaxTerms || !out) return MODA_EINVAL;
    AsmTerms a;
    a.n = n_terms;
    a.total_wt = total_wt;
    long long most = 0;
    for (int t = 0; t < n_terms; ++t) {
        const moda_asm_term& q = terms[t];
        if (!q.x && !g) return MODA_EINVAL;
        if (q.n < 1 || q.k < 1 || q.n > (1 << 24) || q.mask_kind < 0 || q.mask_kind > 3 || (q.mask_kind && !q.mask)) return MODA_EINVAL;
        a.t[t] = q;
        if (q.n * q.k > most) most = q.n * q.k;
    }
    for (int t = n_terms; t < kMaxTerms; ++t) a.t[t] = moda_asm_term{};
    if (g) hipLaunchKernelGGL(loss_asm_bwd_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)n_terms), dim3(256), 0, (hipStream_t)stream, a, (const float*)out, g);
    else hipLaunchKernelGGL(loss_asm_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a, out);
    return (int)hipGetLastError();
}
