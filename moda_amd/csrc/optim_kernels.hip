// The optimiser stage of the reference's training step, device-resident (nnutils/train_utils.py:226-290, :967-969):
// torch.optim.AdamW over 22 parameter groups driven by OneCycleLR with per-group peaks, then optimizer.zero_grad().  The
// learning rates are computed ON THE DEVICE from a device step counter, so a captured graph follows the schedule when it is
// replayed (torch's scheduler.step() is host code: a replayed graph keeps the rate it was captured with).  Memory-bound --
// 4 fp32 reads and 3 writes per element (4 writes with zero_grad) -- no MFMA.  Two launches, no host sync, no allocation.
//
//   tables     as clip_kernels.hip: a segment is one parameter tensor WITH a gradient (pointer to p, pointer to g, numel, group,
//              offset of its moments in the two flat state buffers); a chunk is MODA_CLIP_CHUNK floats of ONE segment.
//   prepare    one workgroup.  Reads the step counter t (int64), lanes 0..G-1 compute their group's OneCycleLR rate in float64
//              with torch's arithmetic (two phases ending at pct_start * total_steps - 1 and total_steps - 1, linear anneal,
//              initial = max / div_factor, min = initial / final_div_factor; torch's formula as it is up to t == total_steps, the
//              slight extrapolation there included).  Past total_steps torch raises; nothing can raise from a graph, so the rate of
//              total_steps is held and status[0] counts the overrun steps.  lr[0..G) = the rate this step applies, lr[G..2G) = the
//              rate `param_groups[g]['lr']` holds after scheduler.step() (what the reference logs into aux_out), both rounded to
//              fp32.  Then one lane per segment: k = ++seg_step[s] (torch keeps `step` per parameter and skips a parameter whose
//              grad is None, so k is per segment) and the three scalar factors 1 - lr * wd, lr / (1 - beta1^k), sqrt(1 - beta2^k),
//              each computed in float64 and rounded ONCE to fp32 -- as torch's single-tensor AdamW does with Python doubles.
//   apply      one workgroup per chunk; lane t owns the quads t, t + 256, t + 512, t + 768 of the chunk (one float4 access per
//              array whose chunk start is 16-byte aligned, bounds-checked scalars otherwise and in the tail quad -- the clipper's
//              element-to-lane map).  Per element, every operation rounded to fp32 (contraction is off for this file; divide
//              and square root are the correctly rounded ones):
//                  p  = p * f_decay
//                  m  = m + w1 * (g - m)                    w1 = (float)(1 - beta1)          (lerp_)
//                  v  = v * b2;  v = v + (w2 * g) * g       b2 = (float)beta2, w2 = (float)(1 - beta2)   (mul_, addcmul_)
//                  d  = sqrt(v) / f_bc2 + eps
//                  p  = p - (f_step * m) / d                                                 (addcdiv_, value = -step_size)
//              zero_grad: literal zeros over the gradient just read (optimizer.zero_grad() without a second pass).
// The stage does not look at the clipper's status: after a rejected step, and in a frozen group, the gradients are zeros and
// AdamW still steps (decay and momentum move the parameters, `step` advances), exactly as the reference does.
// No float atomics, no reductions: the bits do not depend on the run.  Device memory is written only by plain vector stores.
// Chunk and segment indices are int32; element offsets in 64 bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_hip.h"
#include "lanes.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = MODA_CLIP_CHUNK;
constexpr int kQuads = kChunk / 4 / kBlock;          // quads per lane
constexpr int kMaxGroups = MODA_OPTIM_MAX_GROUPS;
static_assert(kQuads * 4 * kBlock == kChunk, "a chunk is a whole number of quads per lane");
static_assert(kMaxGroups <= kBlock, "one lane per group");

struct Hyper {
    int64_t total_steps;
    double pct_start, div_factor, final_div_factor, beta1, beta2, weight_decay;
};

// torch.optim.lr_scheduler.OneCycleLR.get_lr (three_phase False, anneal_strategy 'linear') at step_num, in its operations
DEVINL double one_cycle(double max_lr, const Hyper& h, int64_t step_num) {
    const double initial_lr = max_lr / h.div_factor, min_lr = initial_lr / h.final_div_factor;
    const double end0 = h.pct_start * (double)h.total_steps - 1.0, end1 = (double)h.total_steps - 1.0;
    const double s = (double)step_num;
    if (s <= end0) {
        const double pct = (s - 0.0) / (end0 - 0.0);
        return (max_lr - initial_lr) * pct + initial_lr;
    }
    const double pct = (s - end0) / (end1 - end0);
    return (min_lr - max_lr) * pct + max_lr;
}

__global__ __launch_bounds__(kBlock) void adamw_prepare_kernel(const double* __restrict__ max_lr, int G, Hyper h,
                                                               const int32_t* __restrict__ seg_group, int n_seg,
                                                               int64_t* __restrict__ step, int64_t* __restrict__ seg_step,
                                                               float* __restrict__ lr, float* __restrict__ seg_fac,
                                                               int32_t* __restrict__ status) {
    __shared__ double lr_s[kMaxGroups];
    const int t = threadIdx.x;
    const int64_t t_now = step[0];                                           // every lane reads it before lane 0 writes it
    const int64_t t_use = t_now < 0 ? 0 : (t_now > h.total_steps ? h.total_steps : t_now);
    const int64_t t_next = t_use + 1 > h.total_steps ? h.total_steps : t_use + 1;
    if (t < G) {
        const double a = one_cycle(max_lr[t], h, t_use);
        lr_s[t] = a;
        lr[t] = (float)a;
        lr[G + t] = (float)one_cycle(max_lr[t], h, t_next);
    }
    __syncthreads();
    for (int s = t; s < n_seg; s += kBlock) {
        const int g = seg_group[s];
        const int64_t k = seg_step[s] + 1;
        float f0 = 1.f, f1 = 0.f, f2 = 1.f;                                  // a segment without a group: p, m, v barely move
        if (g >= 0 && g < G) {
            const double a = lr_s[g], kd = (double)k;
            f0 = (float)(1.0 - a * h.weight_decay);
            f1 = (float)(a / (1.0 - pow(h.beta1, kd)));
            f2 = (float)sqrt(1.0 - pow(h.beta2, kd));
        }
        seg_fac[3 * s] = f0;
        seg_fac[3 * s + 1] = f1;
        seg_fac[3 * s + 2] = f2;
        seg_step[s] = k;
    }
    if (t == 0) {
        step[0] = t_now + 1;
        const int32_t over = status[0];
        if (t_now > h.total_steps && over < 2147483647) status[0] = over + 1;
    }
}

struct Tables {
    float* const* seg_p;
    float* const* seg_g;
    const int64_t* seg_numel;
    const int32_t* seg_group;
    const int64_t* seg_moff;
    int32_t n_seg;
    const int32_t* chunk_seg;
    const int64_t* chunk_off;
    int32_t G;
    int64_t n_state;
};

struct Arr {
    float* p;
    bool aligned;
};

DEVINL Arr arr(float* p) { return Arr{p, ((uintptr_t)p & 15) == 0}; }

// quad q of a chunk of n elements: v[0..cnt), cnt = the elements of the quad inside the chunk
DEVINL int load_quad(const Arr& a, int n, int q, float v[4]) {
    const int e = 4 * q;
    if (a.aligned && e + 4 <= n) {
        const float4 t = *reinterpret_cast<const float4*>(a.p + e);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        return 4;
    }
    const int cnt = n - e < 4 ? (n - e > 0 ? n - e : 0) : 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < cnt ? a.p[e + j] : 0.f;
    return cnt;
}

DEVINL void store_quad(const Arr& a, int n, int q, const float v[4]) {
    const int e = 4 * q;
    if (a.aligned && e + 4 <= n) {
        *reinterpret_cast<float4*>(a.p + e) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (e + j < n) a.p[e + j] = v[j];
}

__global__ __launch_bounds__(kBlock) void adamw_apply_kernel(Tables T, const float* __restrict__ seg_fac, float* __restrict__ exp_avg,
                                                             float* __restrict__ exp_avg_sq, float w1, float b2, float w2, float eps,
                                                             int zero_grad) {
    const int c = blockIdx.x, t = threadIdx.x;
    // a table entry that does not describe a range of a segment and of the state buffers is skipped, never followed
    const int s = T.chunk_seg[c];
    if (s < 0 || s >= T.n_seg) return;
    const int64_t numel = T.seg_numel[s], off = T.chunk_off[c], moff = T.seg_moff[s];
    const int g = T.seg_group[s];
    float* const pb = T.seg_p[s];
    float* const gb = T.seg_g[s];
    if (!pb || !gb || off < 0 || off >= numel || g < 0 || g >= T.G || moff < 0 || moff > T.n_state || numel > T.n_state - moff) return;
    const int n = (int)(numel - off < (int64_t)kChunk ? numel - off : (int64_t)kChunk);
    const Arr P = arr(pb + off), Gr = arr(gb + off), M = arr(exp_avg + moff + off), V = arr(exp_avg_sq + moff + off);
    const float f_decay = seg_fac[3 * s], f_step = seg_fac[3 * s + 1], f_bc2 = seg_fac[3 * s + 2];
    const float zeros[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < kQuads; ++i) {
        const int q = t + kBlock * i;
        if (4 * q >= n) break;
        float p[4], gr[4], m[4], v[4];
        const int cnt = load_quad(P, n, q, p);
        load_quad(Gr, n, q, gr);
        load_quad(M, n, q, m);
        load_quad(V, n, q, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= cnt) break;
            const float p1 = p[j] * f_decay;
            const float m1 = m[j] + w1 * (gr[j] - m[j]);
            float v1 = v[j] * b2;
            v1 = v1 + (w2 * gr[j]) * gr[j];
            const float d = __fadd_rn(__fdiv_rn(sqrtf(v1), f_bc2), eps);
            p[j] = p1 - __fdiv_rn(f_step * m1, d);
            m[j] = m1;
            v[j] = v1;
        }
        store_quad(P, n, q, p);
        store_quad(M, n, q, m);
        store_quad(V, n, q, v);
        if (zero_grad) store_quad(Gr, n, q, zeros);
    }
}

}   // namespace

extern "C" int moda_adamw_step(float* const* seg_p, float* const* seg_g, const int64_t* seg_numel, const int32_t* seg_group,
                               const int64_t* seg_moff, int32_t n_seg, const int32_t* chunk_seg, const int64_t* chunk_off,
                               int32_t n_chunks, const double* max_lr, int32_t G, int64_t total_steps, double pct_start,
                               double div_factor, double final_div_factor, double beta1, double beta2, double eps,
                               double weight_decay, int64_t* step, int64_t* seg_step, float* exp_avg, float* exp_avg_sq,
                               int64_t n_state, float* lr, float* seg_fac, int32_t* status, int32_t zero_grad, void* stream) {
    if (n_seg < 0 || n_chunks < 0 || G < 1 || G > kMaxGroups || total_steps < 1 || n_state < 0) return MODA_EINVAL;
    if (!max_lr || !step || !lr || !status) return MODA_EINVAL;
    if (!(div_factor > 0.0) || !(final_div_factor > 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return MODA_EINVAL;
    // a phase of no length divides by zero (torch raises ZeroDivisionError at the step that meets it)
    const double end0 = pct_start * (double)total_steps - 1.0, end1 = (double)total_steps - 1.0;
    if (!(pct_start >= 0.0 && pct_start <= 1.0) || end0 == 0.0 || end1 == end0) return MODA_EINVAL;
    if (n_seg > 0 && (!seg_group || !seg_step || !seg_fac)) return MODA_EINVAL;
    if (n_chunks > 0 && (!seg_p || !seg_g || !seg_numel || !seg_moff || !chunk_seg || !chunk_off || !exp_avg || !exp_avg_sq
                         || n_seg < 1))
        return MODA_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Hyper h{total_steps, pct_start, div_factor, final_div_factor, beta1, beta2, weight_decay};
    hipLaunchKernelGGL(adamw_prepare_kernel, dim3(1), dim3(kBlock), 0, st, max_lr, (int)G, h, seg_group, (int)n_seg, step, seg_step,
                       lr, seg_fac, status);
    if (n_chunks > 0) {
        const Tables T{seg_p, seg_g, seg_numel, seg_group, seg_moff, n_seg, chunk_seg, chunk_off, G, n_state};
        hipLaunchKernelGGL(adamw_apply_kernel, dim3((unsigned)n_chunks), dim3(kBlock), 0, st, T, (const float*)seg_fac, exp_avg,
                           exp_avg_sq, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (int)zero_grad);
    }
    return (int)hipGetLastError();
}
