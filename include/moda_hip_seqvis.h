/* moda_hip_seqvis.h -- the mesh-sequence rendering entries of libmoda_hip.so: what scripts/visualize/render_vis.py:246-511 does per
 * frame around pyrender -- the viewpoint cameras, projection with behind-the-camera culling, vertex normals, base colours, Lambert
 * shading with the bone layer composited over the body, the overlay on the input frame, the crop to the frame and the resize to
 * the video's width -- for all frames of a MeshSequence at once; moda_amd/csrc/seqvis_kernels.hip, moda_amd/seq_render.py.  The
 * rasteriser between projection and shading is moda_raster_fwd (moda_hip.h), unchanged.
 * A fourth header in the regular shape of moda_hip.h (moda_amd/abi.py parses all four): the entries of moda_hip.h, moda_hip_vis.h
 * and moda_hip_cams.h are unchanged and moda_abi_version() stays 11.  Nothing allocates, synchronises or reads back, every launch
 * goes to `stream`.  No float atomics: every floating-point sum has one fixed order, so the same input gives the same bits on
 * every run and for every split of the frames into calls.  The only atomics are int32 adds into `status` (and the per-frame
 * silhouette counters that feed it).  Contraction is off in the float64 and the projection arithmetic. */
#ifndef MODA_HIP_SEQVIS_H
#define MODA_HIP_SEQVIS_H
#include "moda_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MODA_SEQVIS_BLOCK 256          /* lanes of every workgroup of this file */
#define MODA_SEQVIS_REC_FLOATS 8       /* a vertex record, one 32-byte line: r, g, b (0..255), nx, ny, nz (camera frame, unit), 0, 0 */
/* the int32 status word (MODA_SEQVIS_STATUS_WORDS), counts that the entries ADD to: the caller zeroes it */
#define MODA_SEQVIS_STATUS_WORDS 8
#define MODA_SEQVIS_DROPPED 0          /* (view, face) pairs dropped because a corner lies at Z <= 0 */
#define MODA_SEQVIS_NONFINITE 1        /* (view, vertex) pairs whose projected x, y or z is not finite */
#define MODA_SEQVIS_NAN_ERROR 2        /* (frame, vertex) error values that are NaN (coloured 0, 0, 0) */
#define MODA_SEQVIS_EMPTY 3            /* frames whose silhouette inside the H x W window is empty */
#define MODA_SEQVIS_BAD_INDEX 4        /* (view, face) pairs that index a vertex outside [0, V) (skipped, not counted as dropped) */
/* moda_seqvis_cams' viewpoint */
#define MODA_SEQVIS_VP_STATIC (-1)     /* --vp -1: the first frame's camera */
#define MODA_SEQVIS_VP_CANONICAL (-2)  /* --vp -2: Rodrigues(0, pi/3, 0) Rodrigues(pi, 0, 0), the first frame's depth */
/* moda_seqvis_records' colour source */
#define MODA_SEQVIS_COLOR_U8 0         /* floor(0.6 c) of uint8 colours, as the integer (3 c) / 5 */
#define MODA_SEQVIS_COLOR_CONST 1      /* one value for every channel of every vertex */
#define MODA_SEQVIS_COLOR_ERROR 2      /* a 256-entry colour table indexed by 5 * error under matplotlib's rule for floats */

/* moda_seqvis_cams: render_vis.py:259-322 for F frames in one launch, a workgroup a frame, composed in float64 from the fp32
 * inputs and rounded once.  rtk (F,4,4) = [R | T ; fx fy px py].  verts (Fv,V,3), Fv = F (a frame's own vertices) or 1 (the same
 * vertices in every view): only vp 1 and 2 read them, for the mean, a float64 sum in a fixed order (a lane's vertices in index
 * order, the xor butterfly of its wave, the waves in index order) divided by V.
 * turntable != 0 (--freeze / --rest): the frame's camera is first replaced by Rodrigues(0, 2 pi f / F, 0) R_0, t = (0, 0, t_0z),
 * K = (fx_0, fy_0, W / 2, H / 2).  Then the viewpoint: vp 0 keeps it; vp 1 / 2: R' = Rodrigues(0, pi/2, 0) / Rodrigues(pi/2, 0, 0)
 * times R and t_xy = -(R' mean)_xy; MODA_SEQVIS_VP_STATIC: R' = (R_0 R^T) R, t = t_0, K = K_0 with the principal point passed
 * through the reference's k / W_0 * W_i at W_0 = W_i; MODA_SEQVIS_VP_CANONICAL: R' = (C R^T) R, t = (0, 0, t_0z), K likewise.
 * cams (F,4,4): the cameras to render with.  ctrajs (F,4,4): [R' | t] over K * (out_width / W) (:502-509, with the row's own fx
 * and fy).  MODA_ESHAPE: F or V < 1, F > 2^24, Fv not 1 or F, V >= 2^31, W, H or out_width < 1, vp outside -2..2. */
int moda_seqvis_cams(const float* rtk, const float* verts, int64_t F, int64_t Fv, int64_t V, int32_t vp, int32_t turntable,
                     int64_t W, int64_t H, int64_t out_width, float* cams, float* ctrajs, void* stream);

/* moda_seqvis_project: n views in one launch.  verts (Fv,V,3), Fv = n or 1; cams (n,4,4); faces (Nf,3) int32.  Per (view, vertex),
 * in fp32 with every operation rounded once: X = ((r0 x + r1 y) + r2 z) + t (obj_to_cam), Zs = Z, or 1e-12 when |Z| < 1e-12,
 * u = fx X / Zs + px, v = fy Y / Zs + py, ndc = (u (2 / S) - 1, -(v (2 / S) - 1), Z), the frame moda_raster_fwd documents.  cam
 * (n,V,3) takes (X, Y, Z), ndc (n,V,3) the above; a workgroup stages its 256 rows in LDS and writes them as whole lines.
 * view_faces (n,Nf,3): the face where its three indices lie in [0, V) and every corner has Z > 0, else (-1, -1, -1), which
 * moda_raster_fwd skips; nothing is compacted.  status[MODA_SEQVIS_DROPPED], [MODA_SEQVIS_BAD_INDEX] and [MODA_SEQVIS_NONFINITE]
 * are added to.  MODA_ESHAPE: n, V, Nf or S < 1, S > 32768, n V or n Nf >= 2^31 / 3, Fv not 1 or n. */
int moda_seqvis_project(const float* verts, const float* cams, const int32_t* faces, int64_t n, int64_t Fv, int64_t V, int64_t Nf,
                        int64_t S, float* cam, float* ndc, int32_t* view_faces, int32_t* status, void* stream);

/* moda_seqvis_records: the vertex records of n views in one launch, one lane a (view, vertex).  Normal: the area-weighted vertex
 * normal in the camera frame, the fp32 cross products (v1 - v0) x (v2 - v0) of the incident faces that view_faces keeps, added in
 * ascending face order, divided by max(|n|, 1e-12); zero for a vertex of no face.  csr_off (V + 1) and csr_ent: entry e = 3 face
 * + corner of every incident corner of vertex v at csr_ent[csr_off[v] .. csr_off[v + 1]), ascending.
 * Colour by color_mode: MODA_SEQVIS_COLOR_U8: colors_u8 (Fc,V,3) bytes, Fc = n or 1; MODA_SEQVIS_COLOR_CONST: color_const;
 * MODA_SEQVIS_COLOR_ERROR: table (256,3) fp32 at index (int)(x 256), x = 5 error (fp32), the first entry for x < 0, the last for
 * x >= 1, (0, 0, 0) and a count in status[MODA_SEQVIS_NAN_ERROR] for NaN; error (n,V).
 * rec (n,V,MODA_SEQVIS_REC_FLOATS), 32-byte aligned rows written as two 16-byte stores.  MODA_ESHAPE: n or V < 1, n V >= 2^28. */
int moda_seqvis_records(const float* cam, const int32_t* view_faces, const int32_t* csr_off, const int32_t* csr_ent, int64_t n,
                        int64_t V, int64_t Nf, int32_t color_mode, const uint8_t* colors_u8, int64_t Fc, float color_const,
                        const float* error, const float* table, float* rec, int32_t* status, void* stream);

/* moda_seqvis_shade: one lane per pixel of the H x W window (rows 0..H-1, columns 0..W-1) of n S x S rasters.  Body layer:
 * face_idx (n,S,S), bary (n,S,S,3), zbuf (n,S,S) of moda_raster_fwd, faces (Nf,3), rec (n,V,8), cam (n,V,3).  Bone layer: the same
 * seven with a `b`, or face_idx_b NULL for none.  Per layer, where face_idx is a face of [0, Nf): rgb = b0 c0 + b1 c1 + b2 c2 of
 * the corners' records; lambert = |n_z| / max(|n|, 1e-12) of the interpolated record normals (smooth != 0) or of the face's
 * (v1 - v0) x (v2 - v0) in the camera frame; the layer's colour is min(max(rgb (0.4 + lambert), 0), 255).  Composite: bone alone
 * where the body is absent or zbuf_b < zbuf; body alone where the bone is absent; else opacity body + (1 - opacity) bone.
 * depth = the smaller zbuf of the layers present, 0 for none.  color (n,H,W,3) bytes: the truncated colour, 0 for none; with
 * overlay (n,H,W,3) bytes, every pixel becomes (c + o) / 2 rounded half to even; pixel (0, 0) of every frame is 0.
 * sil (n,H,W) int16 (a void* here: the header's types know no int16) = 100 (depth > 0).  sil_count (n) int32 is ADDED the frame's number of silhouette pixels.
 * MODA_ESHAPE: n, H, W < 1, H or W > S, S > 32768, n S S >= 2^31. */
int moda_seqvis_shade(const int32_t* face_idx, const float* bary, const float* zbuf, const int32_t* faces, const float* rec,
                      const float* cam, int64_t V, int64_t Nf, const int32_t* face_idx_b, const float* bary_b, const float* zbuf_b,
                      const int32_t* faces_b, const float* rec_b, const float* cam_b, int64_t Vb, int64_t Nfb, int64_t n, int64_t S,
                      int64_t H, int64_t W, int32_t smooth, float opacity, const uint8_t* overlay, uint8_t* color, float* depth,
                      void* sil, int32_t* sil_count, void* stream);

/* moda_seqvis_resize: color (n,H,W,3) bytes and sil (n,H,W) int16 -> frames (n,h,w,3) bytes and refsil (n,h,w) int16, bilinear
 * with half-pixel centres: source x = (col + 0.5) (W / w) - 0.5 in fp32 (W / w rounded once from float64), the two neighbours
 * clamped to the image, weights and sums in fp32, rounded half to even.  status[MODA_SEQVIS_EMPTY] is added the frames whose
 * sil_count is 0.  MODA_ESHAPE: any size < 1, n H W or n h w >= 2^31 / 3. */
int moda_seqvis_resize(const uint8_t* color, const void* sil, const int32_t* sil_count, int64_t n, int64_t H, int64_t W,
                       int64_t h, int64_t w, uint8_t* frames, void* refsil, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MODA_HIP_SEQVIS_H */
