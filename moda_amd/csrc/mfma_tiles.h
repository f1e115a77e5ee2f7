// The MFMA tile vocabulary of the bf16-operand training kernels (gemm_bf16.hip, gemm_x3.hip, bwd64_chain.hip, bwd256_fused.hip;
// the bf16 words also train_kernels.hip, loss_kernels.hip): bf16 pack / unpack, the k-slow and k-fast LDS images with their
// fragment reads (modelled lane by lane in tests/test_gemm3_layout.py), and the parts of the 2 x 2-wave tile engine that
// gemm_bf16.hip and gemm_x3.hip share -- tile placement, k schedule, the atomic (dW form) epilogue and its host-side planner.
// Included by those six files only; DEVINL and the alignment test al16 come from lanes.h through moda_dev.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "moda_dev.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// ---- bf16 words --------------------------------------------------------------------------------------------------------------
DEVINL unsigned pk2(float lo, float hi) {       // two floats -> two bf16 (round to nearest even), lo in the low half
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
    const f32x2_ t = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(t, bf16x2_));
}
DEVINL uint4 pack8(const float4& a, const float4& b) { return make_uint4(pk2(a.x, a.y), pk2(a.z, a.w), pk2(b.x, b.y), pk2(b.z, b.w)); }
DEVINL float bflo(unsigned w) { return __builtin_bit_cast(float, w << 16); }            // the low / high bf16 of a word, as a float
DEVINL float bfhi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }
// the two bf16 of vw kept where those of mw are > 0:  bf16 > 0  <=>  its 16 bits, as a signed integer, > 0
DEVINL unsigned keep_pos(unsigned vw, unsigned mw) {
    const unsigned lo = ((short)(mw & 0xffffu) > 0) ? 0x0000ffffu : 0u;
    const unsigned hi = ((int)mw > 0xffff) ? 0xffff0000u : 0u;      // high half positive and nonzero
    return vw & (lo | hi);
}

// ---- the k-slow ([k][T], read with ds_read_b64_tr_b16) and k-fast ([row][k] padded, read with ds_read_b128) LDS images -----
// chunk swizzle of a [k][T] bf16 image (rows of 2T bytes, 16-byte chunks): the four rows one transposing read takes
// (4n .. 4n+3, 64 bytes each per 32-lane half) land in four different 64-byte bank groups
template <int T>
DEVINL int ks_sw(int row) { return T == 128 ? ((row & 3) << 2) : (((row >> 1) & 1) << 2); }

// Per-lane base of the transposing reads of the 32-wide block at column `cb` of a [k][T] image, 16-lane group gq = g & 1 of
// lane half h: lane 4q+p supplies row (16u + 8h + 4e) + q, elements 16 gq + 4p .. +3 of the block; it receives, for its own
// column (lane & 31), the k = 8h + 4e + (0..3) of k-step u -- elements 4e .. 4e+3 of the MFMA operand.
template <int T>
DEVINL int tr_base(int lane, int cb) {
    const int h = lane >> 5, g = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
    const int ch = cb / 8 + 2 * (g & 1) + (p4 >> 1);
    return (8 * h + q4) * (T * 2) + 16 * (ch ^ ks_sw<T>(q4)) + 8 * (p4 & 1);
}
// k-fast image, rows of `stride` bytes: the lane reads its own row's eight k = 16u + 8h .. +7 (at + 32 u) with one 16-byte read
DEVINL int kf_base(int lane, int rb, int stride) { return (rb + (lane & 31)) * stride + 16 * (lane >> 5); }

// one MFMA operand from two transposing reads, at byte offsets lo_off / hi_off (four k rows apart) from `base`
DEVINL bf16x8 tr_frag(const unsigned char* base, int lo_off, int hi_off) {
    typedef s16x4 __attribute__((address_space(3))) lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + lo_off));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(base + hi_off));
    union { struct { s16x4 a, b; } s; bf16x8 v; } o;
    o.s.a = lo;
    o.s.b = hi;
    return o.v;
}
// k-step u of an image with rows of rb bytes, from the lane base `off` (tr_base)
DEVINL bf16x8 tr_frag(const unsigned char* base, int off, int rb, int u) { return tr_frag(base + off, (16 * u) * rb, (16 * u + 4) * rb); }

// ---- the tile engine of gemm_bf16.hip and gemm_x3.hip: 4 waves as 2 x 2 on a TR x TC tile -----------------------------------
// dispatch id -> tile (and k slice).  Tiles that share the rows of a long operand get dispatch ids 8 apart: one XCD, one L2
// (workgroups are dealt round-robin over the 8 XCDs, each with its own L2: what one XCD has fetched, another fetches again)
template <bool ATOMIC>
DEVINL void place_tile(unsigned lid, unsigned gr, unsigned gc, int splits, unsigned& tr_idx, unsigned& tc_idx, unsigned& slice) {
    slice = 0;
    if (ATOMIC) {
        // the tiles of one k slice read the same rows of dZ and X: dispatch ids 8 apart, so that one XCD's L2 serves the
        // second reader of every chunk (measured without: every operand byte crosses the fabric once per tile column / row)
        const unsigned nt = gr * gc;
        unsigned t = lid % nt;
        slice = lid / nt;
        if ((splits & 7) == 0) {
            t = (lid >> 3) % nt;
            slice = (lid / (8 * nt)) * 8 + (lid & 7);
        }
        tr_idx = t % gr;
        tc_idx = t / gr;
    } else {
        tr_idx = lid % gr;
        tc_idx = lid / gr;
        if (gr > 1 && (gc & 7) == 0) {
            const unsigned span = 8 * gr, r = lid % span;
            tr_idx = r >> 3;
            tc_idx = (lid / span) * 8 + (r & 7);
        }
    }
}

// split over k: engine e of E = splits x NG (slice s, group g: e = s NG + g) takes the k-tiles e, e + E, e + 2E, ...:
// engines that run at the same time read neighbouring KT-row pieces of the operands (measured the same as one
// contiguous range per engine; kept because it makes the ranges independent of K)
struct KSched { int kstep, kbeg, nit; };
template <int KT, int NG>
DEVINL KSched k_schedule(int K, int splits, int slice, int grp) {
    KSched s;
    s.kstep = KT * splits * NG;
    s.kbeg = (slice * NG + grp) * KT;
    s.nit = (K - slice * NG * KT + s.kstep - 1) / s.kstep;      // trips of group 0, the longest: every group runs as many
    return s;
}

template <int NI, int NJ>
DEVINL void clear_acc(f32x16 (&acc)[NI][NJ]) {
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// The epilogue of the dW form: C (r, c) at r * ldc + c += T with fp32 atomics, xsum[r] += the staged column sums (or null).
// NG: wave groups per workgroup.  Each group of 4 waves is a complete 2 x 2 tile engine with its own LDS stage and
// its own k-tiles; the groups' accumulators are summed through LDS before ONE set of atomics leaves the workgroup.  The
// atomics of all workgroups land on the same R x C addresses and serialise there (~37 ns per workgroup whatever the tile:
// 19 of the 23 us of a 64 x 64 product at 512 workgroups), while the stream needs many k-tiles in flight: NG groups give
// the memory parallelism of NG workgroups at the atomic cost of one.
// xsum8: the thread's sums of its staged 16-byte chunk of X (chunk column tid % XCPR of rows tid / XCPR + XRPP e of every k-tile).
// C/D map: lane l register r -> T row (r&3) + 8(r>>2) + 4(l>>5), T column l & 31
template <int TR, int TC, int NG, int XCPR, int XRPP>
DEVINL void epi_atomic(f32x16 (&acc)[TR / 64][TC / 64], const float (&xsum8)[8], unsigned char* lds, int grp, int tid, float* C,
                       long long ldc, float* xsum, long long r0, long long c0, int R, int Cn) {
    constexpr int NI = TR / 64, NJ = TC / 64, NREG = NI * NJ * 16;
    const int lane = tid & 63, wave = tid >> 6, h = lane >> 5;
    const int wr = (wave >> 1) * (TR / 2), wc = (wave & 1) * (TC / 2);
    const int xch = tid % XCPR, xrow = tid / XCPR;
    if (NG > 1) {       // sum the groups' partial tiles into group 0 (lane-linear fp32 images in the now idle stage LDS)
        float* part = (float*)lds;
        if (grp > 0) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) part[(((grp - 1) * NREG) + (i * NJ + j) * 16 + r) * 256 + tid] = acc[i][j][r];
        }
        __syncthreads();
        if (grp == 0) {
#pragma unroll
            for (int g2 = 1; g2 < NG; ++g2)
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc[i][j][r] += part[(((g2 - 1) * NREG) + (i * NJ + j) * 16 + r) * 256 + tid];
        }
        if (xsum != nullptr) {
            __syncthreads();
            float* red = (float*)lds;
#pragma unroll
            for (int e = 0; e < 8; ++e) red[((grp * 256) + xrow * XCPR + xch) * 8 + e] = xsum8[e];
            __syncthreads();
            if (grp == 0 && tid < TR) {
                float sm = 0.f;
                for (int rw = 0; rw < NG * XRPP; ++rw) sm += red[(rw * XCPR + (tid >> 3)) * 8 + (tid & 7)];
                if (r0 + tid < R) atomicAdd(xsum + r0 + tid, sm);
            }
        }
        if (grp != 0) return;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const long long c = c0 + wc + 32 * j + (lane & 31);
            if (c >= Cn) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long rr = r0 + wr + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (rr < R) atomicAdd(C + rr * ldc + c, acc[i][j][r]);
            }
        }
    if (NG == 1 && xsum != nullptr) {      // threads with the same chunk column hold partial sums of the same eight r
        float* red = (float*)lds;
#pragma unroll
        for (int e = 0; e < 8; ++e) red[(xrow * XCPR + xch) * 8 + e] = xsum8[e];
        __syncthreads();
        if (tid < TR) {
            float s = 0.f;
            for (int rw = 0; rw < XRPP; ++rw) s += red[(rw * XCPR + (tid >> 3)) * 8 + (tid & 7)];
            if (r0 + tid < R) atomicAdd(xsum + r0 + tid, s);
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
// The launch plan of the dW form (R x Cn result, K long): 128 x 128 tiles, or 64 x 64 for the 64-wide nets, and the split
// over k: one workgroup per CU (NG = 2 | 4 wave groups each), every engine with at least two k-tiles of KT
struct DwPlan { unsigned gr, gc, splits; bool big; };
inline DwPlan plan_dw_splits(long long R, long long Cn, long long K, int KT, long long target_override) {
    DwPlan p;
    p.big = R > 64 || Cn > 64;
    const int T = p.big ? 128 : 64;
    p.gr = (unsigned)((R + T - 1) / T); p.gc = (unsigned)((Cn + T - 1) / T);
    const long long target = target_override > 0 ? target_override : (p.big ? 256 : 128);    // measured best (64 .. 512 swept)
    const int ng = p.big ? 2 : 4;
    const long long nkt = (K + KT - 1) / KT;
    long long splits = target / ((long long)p.gr * p.gc);
    if (splits > nkt / (2 * ng)) splits = nkt / (2 * ng);
    if (splits < 1) splits = 1;
    if (splits >= 8) splits &= ~7LL;              // whole groups of 8 slices: the XCD placement in the kernel
    p.splits = (unsigned)splits;
    return p;
}

}   // namespace
