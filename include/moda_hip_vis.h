/* moda_hip_vis.h -- the evaluation-frame entries of libmoda_hip.so: the canvases, grids, flow colours and 8-bit frames that
 * v2s_trainer.eval() builds after every epoch (nnutils/train_utils.py:496-520, :1482-1504, nnutils/vis_utils.py:5-16,
 * third_party/ext_utils/flowlib.py:86-214, utils/io.py:242-258; moda_amd/csrc/evalvis_kernels.hip, moda_amd/eval_frames.py).
 * A header of its own, in the regular shape of moda_hip.h (moda_amd/abi.py parses both): the entries of moda_hip.h are unchanged
 * and moda_abi_version() stays 11.  Nothing allocates, synchronises or reads back, every launch goes to `stream`.  No float
 * atomics: the extrema are integer maxima over an order-preserving map of the float bits, so the same bits come out on every run
 * and for every tiling; the status counters are integer adds. */
#ifndef MODA_HIP_VIS_H
#define MODA_HIP_VIS_H
#include "moda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MODA_VIS_BLOCK 256           /* lanes of every workgroup of this file */
#define MODA_VIS_TILE 2048           /* elements of a key that one workgroup reduces / writes */
#define MODA_VIS_MAX_KEYS 65535      /* rows of an op table (a grid dimension) */
#define MODA_VIS_OP_FIELDS 8         /* int64 fields of an op-table row: [off, n, C, flags, mul_off, 0, 0, 0] */
/* flags of an op-table row: what the value of element e of the key is, and what moda_vis_apply does to it */
#define MODA_VIS_OP_MASK 1           /* value *= mask nearest-resized to S x S, at the element's frame and pixel */
#define MODA_VIS_OP_MUL 2            /* value *= x[mul_off + e / C], a one-channel key of the same packed buffer */
#define MODA_VIS_OP_SUBMIN 4         /* apply: value -= min */
#define MODA_VIS_OP_SCALE255 8       /* apply: value *= 255 / max (with SUBMIN: 255 / (max - min), the max after the subtraction) */
#define MODA_VIS_OP_UNIT 16          /* apply: value = (value - min) / (max - min) */
#define MODA_VIS_OP_CLAMP01 32       /* apply: value < 0 -> 0, value > 1 -> 1, NaN kept */
#define MODA_VIS_OP_RAD 64           /* minmax only: the key holds n pixels of C >= 2 channels, value = sqrt(u u + v v) of the first two,
                                      * a pixel with |u| or |v| > 1e7 counting as 0 */
/* the int32 status word (4 counters, the caller zeroes them) */
#define MODA_VIS_STATUS_ZERO_DIV 0   /* keys whose SCALE255 / UNIT divisor was 0 */
#define MODA_VIS_STATUS_NAN_EXT 1    /* keys whose minimum or maximum is NaN, or whose row the kernels refused */
#define MODA_VIS_STATUS_SATURATED 2  /* values moda_vis_to_u8 saturated */
#define MODA_VIS_STATUS_NAN_U8 3     /* NaNs moda_vis_to_u8 turned into 0 */

/* moda_vis_minmax: the minimum and maximum of every key of an op table, two launches.  x: one packed fp32 buffer of `total`
 * floats; ops (nkeys, MODA_VIS_OP_FIELDS) int64 in device memory, key k being x[off, off + n C') with C' = 1 but for
 * MODA_VIS_OP_RAD keys (C' = C); max_n >= every n.  Element e of a key belongs to pixel p = e / C, frame p / (S S); its value is
 * x[off + e], times mask[frame, floor(y Sm / S), floor(x Sm / S)] for MODA_VIS_OP_MASK (torch's legacy `nearest`: the scale
 * (float) Sm / S in fp32, the index clamped to Sm - 1), times x[mul_off + p] for MODA_VIS_OP_MUL; each product rounded to fp32.
 * mm (nkeys, 2) = [min, max].  A NaN value makes both NaN; -0 orders below +0.  part: (nkeys, ceil(max_n / MODA_VIS_TILE), 2)
 * int32 of the caller's.  A row that does not lie inside x (or whose frame lies outside the mask_bs masks) is not read through:
 * its extrema are NaN.  status (4) int32: NAN_EXT and ZERO_DIV are counted here.  mask may be NULL when no row has
 * MODA_VIS_OP_MASK (such a row's extrema are NaN then).  MODA_ESHAPE: nkeys outside 1..MODA_VIS_MAX_KEYS, max_n or total outside
 * 1..2^31-1, S or Sm outside 1..46340 when mask is given.  MODA_EINVAL: NULL. */
int moda_vis_minmax(const float* x, int64_t total, const int64_t* ops, int64_t nkeys, int64_t max_n, const float* mask,
                    int64_t mask_bs, int64_t Sm, int64_t S, int32_t* part, float* mm, int32_t* status, void* stream);

/* moda_vis_apply: one pass over every key of the op table: out[off + e] = the value moda_vis_minmax reduced, then in this order
 * SUBMIN and SCALE255 (formed together in float64, (value - min) (255 / d), and rounded to fp32 once: within half an ulp of the
 * float64 value, where the reference's four fp32 roundings leave it up to 2.2 ulp away), UNIT (fp32 throughout, torch's own
 * arithmetic), CLAMP01, with [min, max] = mm[k].  A divisor of 0 gives what IEEE gives (inf, and 0 inf = NaN).  out: `total` floats, the packing of x; what lies between the keys is not written.
 * MODA_VIS_OP_RAD rows and refused rows are skipped.  Shapes and errors as moda_vis_minmax. */
int moda_vis_apply(const float* x, int64_t total, const int64_t* ops, int64_t nkeys, int64_t max_n, const float* mask,
                   int64_t mask_bs, int64_t Sm, int64_t S, const float* mm, float* out, void* stream);

/* moda_flow_color: flow_to_image (flowlib.py:86-214) for N frames of HW pixels of C >= 2 channels -> out (N, HW, 3) uint8.
 * maxrad (N): the frame's maximal radius from moda_vis_minmax (MODA_VIS_OP_RAD); NaN stands for the reference's max(-1, nan) = -1.
 * wheel (55, 3) fp32, the colour wheel.  f64_after_norm != 0: u, v are divided by (double) maxrad + 2^-52 in float64 and radius,
 * angle and fk stay float64, as numpy >= 2 promotes an fp32 flow; 0: the division by the fp32 sum maxrad + 2.220446e-16f, radius,
 * atan2f and fk stay fp32, as numpy < 2 keeps them.  In both the wheel is mixed and floor(255 col) taken in float64, no
 * contraction anywhere.  A pixel with |u| or |v| > 1e7 gives 0, a NaN pixel gives 0.
 * MODA_ESHAPE: N or HW < 1, N > 65535, N HW >= 2^31 / 3, C outside 2..65536.  MODA_EINVAL: NULL. */
int moda_flow_color(const float* flow, int64_t N, int64_t HW, int64_t C, const float* maxrad, const float* wheel,
                    int32_t f64_after_norm, uint8_t* out, void* stream);

/* moda_vis_grid: image_grid (vis_utils.py:5-16): img (N,h,w,c) -> out (row h, col w, c), out[i h + y, j w + x] = img[i col + j, y, x],
 * one thread per output float, which gathers.  MODA_ESHAPE: a size < 1, N < row col, row h col w c >= 2^31.  MODA_EINVAL: NULL. */
int moda_vis_grid(const float* img, int64_t N, int64_t h, int64_t w, int64_t c, int64_t row, int64_t col, float* out, void* stream);

/* moda_vis_to_u8: out (P, E) uint8 = the 8-bit form of frames (N, E)[pick[i]]: with mm (N, 2) given, a frame whose maximum is <= 1
 * is first multiplied by 255 (fp32 product; a NaN maximum is not <= 1).  The conversion truncates toward zero and saturates to
 * [0, 255]; NaN -> 0; values <= -1 or >= 256 are counted in status[SATURATED], NaNs in status[NAN_U8].  A pick outside [0, N)
 * gives 0.  MODA_ESHAPE: a size < 1, N E or P E >= 2^31.  MODA_EINVAL: NULL (mm may be NULL). */
int moda_vis_to_u8(const float* frames, int64_t N, int64_t E, const int32_t* pick, int64_t P, const float* mm, uint8_t* out,
                   int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MODA_HIP_VIS_H */
