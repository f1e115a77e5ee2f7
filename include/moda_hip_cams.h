/* moda_hip_cams.h -- the camera entries of libmoda_hip.so: what the reference does to the pose CNN's cameras after extract_cams
 * (save_cams, nnutils/train_utils.py:744-791), its camera yardstick (align_sim3, nnutils/geom_utils.py:1463-1514;
 * scripts/eval/eval_root.py), the visual-hull centring of prior cameras (visual_hull_align, geom_utils.py:1552-1608) and the
 * camera glyphs of draw_cams (utils/io.py:190-240); moda_amd/csrc/cams_kernels.hip, moda_amd/cams.py.
 * A header of its own, in the regular shape of moda_hip.h (moda_amd/abi.py parses all three): the entries of moda_hip.h and
 * moda_hip_vis.h are unchanged and moda_abi_version() stays 11.  Nothing allocates, synchronises or reads back, every launch goes
 * to `stream`.  No atomics at all: every sum over frames, points and views is a fixed tree (a lane's own items in index order,
 * the xor butterfly of a wave, the waves and then the workgroups in index order), so the same input gives the same bits on every
 * run.  Float64 restatements are followed with contraction off. */
#ifndef MODA_HIP_CAMS_H
#define MODA_HIP_CAMS_H
#include "moda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MODA_CAM_BLOCK 256            /* lanes of every workgroup of this file */
#define MODA_CAM_VIEW_TILE 128        /* views whose camera rows one workgroup of moda_cam_hull_vote stages in LDS at a time */
#define MODA_CAM_PART_FIELDS 5        /* doubles of a workgroup's partial: [selected, sum x, sum y, sum z, non-finite samples] */
#define MODA_CAM_JACOBI_SWEEPS 16     /* at most this many cyclic sweeps over the 4 x 4 matrix sum q q^T */
#define MODA_CAM_MAX_GRID 512         /* lattice points per axis */
#define MODA_CAM_FIT_FIELDS 12        /* doubles of moda_cam_sim3's fit: [R (9, row major), scale, largest, second eigenvalue] */
/* moda_cam_sim3's int32 status word (4) */
#define MODA_CAM_SIM3_ZERO_NORM 0     /* frames whose second translation has norm 0 (the reference divides by it) */
#define MODA_CAM_SIM3_FALLBACK 1      /* 1: inliers were given, none was set, the frame of smallest err_valid was used */
#define MODA_CAM_SIM3_USED 2          /* frames the fit used */
#define MODA_CAM_SIM3_SWEEPS 3        /* Jacobi sweeps taken */
/* moda_cam_hull_apply's int32 status word (4) */
#define MODA_CAM_HULL_NONFINITE 0     /* samples whose image coordinate was not finite (they contributed 0), saturating */
#define MODA_CAM_HULL_EMPTY 1         /* 1: no lattice point was selected, the translations are the input's */
#define MODA_CAM_HULL_SELECTED 2      /* lattice points selected */

/* moda_cam_fill: save_cams' per-frame block (train_utils.py:752-764, :775-776, :788-790) in one launch, one workgroup a video,
 * which walks its frames in chunks of MODA_CAM_BLOCK (a video of any length).  rtk (N,4,4); valid (N) bytes; frame_offset
 * (n_videos + 1) int32, video v holding frames [frame_offset[v], frame_offset[v+1]).  With fill != 0 an invalid frame i of a video
 * that has a valid frame takes the 3 x 3 rotation of the valid frame j of the video that minimises |i - j|, the lower j on a tie
 * (np.argmin): the last valid frame to the left and the first to the right, found by wave ballots and carried across chunks.
 * rtk_out (N,4,4): that rotation, translation * scale (one fp32 product), row 3 copied.  src (N): the frame the rotation came
 * from (i itself when untouched); n_valid (n_videos): valid frames of the video; rows (N, may be NULL) = i + v, the frame's row
 * in a table that keeps one more row per video.  tab_rtk (M,4,4) and tab_rt_raw (M,3,4), both or neither: row i + v takes
 * [R | scaled t] into tab_rt_raw and R into tab_rtk[:3,:3] (translation and row 3 of tab_rtk are not written), and a video's
 * last frame is written a second time into row i + v + 1; a row >= M is not written.  A video whose offsets are not
 * 0 <= lo <= hi <= N is skipped.  MODA_ESHAPE: N or n_videos < 1, N + n_videos >= 2^31.  MODA_EINVAL: NULL, or one table. */
int moda_cam_fill(const float* rtk, const uint8_t* valid, const int32_t* frame_offset, int64_t n_videos, int64_t N, int32_t fill,
                  float scale, float* rtk_out, int32_t* src, int32_t* n_valid, int32_t* rows, float* tab_rtk, float* tab_rt_raw,
                  int64_t M, void* stream);

/* moda_cam_sim3: align_sim3 (geom_utils.py:1463-1514) in one launch of one workgroup, float64 from the fp32 inputs.  roots_a,
 * roots_b (n,4,4).  Per frame dso3 = Rb^T Ra -> the quaternion of scipy's Rotation.from_matrix (the largest of m00, m11, m22 and
 * the trace chooses the branch; normalised), dscale = |ta| / |tb|.  is_inlier (n) bytes or NULL (all frames); when none is set the
 * frame of smallest err_valid (n; the lowest index on a tie, NaN never chosen) is used, err_valid may be NULL when is_inlier is.
 * The mean rotation is scipy's Rotation.mean: the unit eigenvector of the largest eigenvalue of sum q q^T (cyclic Jacobi, one
 * lane, at most MODA_CAM_JACOBI_SWEEPS sweeps), as a matrix; the scale is the mean of dscale.  b_out (n,4,4): Rb' = Rb R,
 * tb' = tb * scale, row 3 copied; the inputs are not written.  so3_err (n) fp32: acos(clamp((trace(Ra Rb'^T) - 1) / 2,
 * +-(1 - 1e-4))) in degrees.  stats (4) double: max, np.median (rank count), mean, unbiased std (NaN for n = 1) of so3_err.
 * fit (MODA_CAM_FIT_FIELDS) double; inlier_used (n) bytes; status (4) int32, all written here.
 * MODA_ESHAPE: n outside 1..2^24.  MODA_EINVAL: NULL, or is_inlier without err_valid. */
int moda_cam_sim3(const float* roots_a, const float* roots_b, const uint8_t* is_inlier, const float* err_valid, int64_t n,
                  float* b_out, double* fit, float* so3_err, double* stats, uint8_t* inlier_used, int32_t* status, void* stream);

/* moda_cam_hull_vote: the voting of visual_hull_align.  rtk (V,4,4), kaug (V,4), masks (V,h,w) fp32 (mask_u8 == 0) or bytes.
 * Every workgroup forms, in fp32 and in the reference's order, each view's kmat = mat2K(K2inv(kaug) K2mat(rtk[3])) and camera
 * centre c = -R^T t, and bound = the mean of |c| over all 3 V entries (a float64 sum rounded once).  Lattice: pts[i] =
 * (float)(i (2 bound / (G - 1)) - bound) in float64, pts[G - 1] = bound; lane p of the launch owns point (pts[i], pts[j], pts[k]),
 * p = (i G + j) G + k.  Per view, in float64: X = R p + t, u = fx X + px Z, v = fy Y + py Z, x = u / (1e-6 + Z), then
 * grid_sample's bilinear sample (align_corners = False, zero padding) of the view's mask; the score is the sum over the views in
 * index order.  A point is selected when score > 0.8 V.  scores (G^3) fp32 or NULL.  part (ceil(G^3 / MODA_CAM_BLOCK),
 * MODA_CAM_PART_FIELDS) double: the workgroup's partial sums.  MODA_ESHAPE: V, h or w < 1, V > 2^20, h w V >= 2^40, G outside
 * 2..MODA_CAM_MAX_GRID.  MODA_EINVAL: NULL. */
int moda_cam_hull_vote(const float* rtk, const float* kaug, const void* masks, int32_t mask_u8, int64_t V, int64_t h, int64_t w,
                       int64_t G, float* scores, double* part, void* stream);

/* moda_cam_hull_apply: one workgroup adds the partials in a fixed tree, centre = the mean of the selected points, and writes
 * rtk_out (V,4,4) = rtk with t = -R (c - centre), c as above (float64, rounded once).  An empty selection leaves t as it was.
 * status (4) int32, all written.  Shapes and errors as moda_cam_hull_vote. */
int moda_cam_hull_apply(const float* rtk, int64_t V, int64_t G, const double* part, float* rtk_out, int32_t* status, void* stream);

/* moda_cam_tnorm_median: out[0] = np.median of the non-zero norms |rtk[i,:3,3]| (fp32 norms of a float64 sum of squares; the
 * median's mean of two in float64; NaN when every norm is 0), one workgroup, by rank count: an element's rank is the number of
 * elements that are smaller, or equal with a lower index.  work: n floats.  MODA_ESHAPE: n outside 1..2^24.  MODA_EINVAL: NULL. */
int moda_cam_tnorm_median(const float* rtk, int64_t n, float* work, float* out, void* stream);

/* moda_cam_glyphs: draw_cams' instancing: out (n, Nv, 3)[i, t] = R_i^T (factor scale[0] tmpl[t]) - R_i^T t_i, float64 rounded
 * once; tmpl (Nv,3) the unit glyph, scale a device float (moda_cam_tnorm_median's).  MODA_ESHAPE: n or Nv < 1, n Nv >= 2^31 / 3. */
int moda_cam_glyphs(const float* rtk, int64_t n, const float* tmpl, int32_t Nv, const float* scale, float factor, float* out,
                    void* stream);

/* moda_cam_links: draw_cams_pair's segments as boxes: out (n, 8, 3), box i spanning the camera centres -R^T t of cam1[i] and
 * cam2[i] with a square section of half-width `half`: corner 4 e + 2 a + b = end e + (2 a - 1) half u + (2 b - 1) half w, u and
 * w unit vectors across the segment (the coordinate axes x, y when the centres coincide).  MODA_ESHAPE: n outside 1..2^24. */
int moda_cam_links(const float* cam1, const float* cam2, int64_t n, float half, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MODA_HIP_CAMS_H */
