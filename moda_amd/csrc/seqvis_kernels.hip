// Mesh-sequence rendering kernels (include/moda_hip_seqvis.h): the stages of scripts/visualize/render_vis.py around the rasteriser,
// for every frame of a sequence, without a host read.
//
//   cams      the viewpoint block in float64, a workgroup a frame; the vertex mean of vp 1 / 2 is a fixed tree (a lane's vertices
//             in index order, wave_add's butterfly, the waves in index order).
//   project   obj_to_cam, pixels and the rasteriser's NDC, one lane a (view, vertex), rows staged in LDS and written as whole
//             lines; the tail of the same grid writes the per-view face lists, a dropped face as (-1, -1, -1).
//   records   one lane a (view, vertex): the area-weighted normal over the vertex's CSR row in ascending face order and the base
//             colour, written as one 32-byte record.
//   shade     one lane a pixel of the H x W window: two layers shaded from their records, composited, overlaid, cropped.
//   resize    bilinear to the video's size.
// Device memory is written by plain vector stores only.  The only atomics are int32 adds of a wave's count into the status word
// and the silhouette counters.  Contraction is off for the whole file: the restatement (tests/seqvis_numpy.py) rounds every
// product and sum on its own.
#include "lanes.h"
#include "moda_hip_seqvis.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = MODA_SEQVIS_BLOCK;
constexpr int kWaves = kBlock / 64;
constexpr int kRec = MODA_SEQVIS_REC_FLOATS;

// adds the number of lanes of the wave with `flag` set to *word: one integer atomic per wave that has any
DEVINL void wave_count(bool flag, int* word) {
    const unsigned long long m = __ballot(flag);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(word, __popcll(m));
}

struct M3 { double m[9]; };

DEVINL M3 mul3(const M3& a, const M3& b) {
    M3 c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c.m[i * 3 + j] = (a.m[i * 3] * b.m[j] + a.m[i * 3 + 1] * b.m[3 + j]) + a.m[i * 3 + 2] * b.m[6 + j];
    return c;
}

DEVINL M3 transpose3(const M3& a) {
    M3 c;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c.m[i * 3 + j] = a.m[j * 3 + i];
    return c;
}

// cv2.Rodrigues of the rotation vector `angle` times the unit axis e_axis: cos I + (1 - cos) e e^T + sin [e]x
DEVINL M3 rodrigues_axis(int axis, double angle) {
    const double c = cos(angle), s = sin(angle);
    M3 r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.m[i] = 0.0;
    r.m[0] = r.m[4] = r.m[8] = c;
    r.m[axis * 4] = c + (1.0 - c);
    const int a = (axis + 1) % 3, b = (axis + 2) % 3;                                // [e]x: (b, a) = +1, (a, b) = -1
    r.m[b * 3 + a] = s;
    r.m[a * 3 + b] = -s;
    return r;
}

// ---- cams ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void seqvis_cams_kernel(const float* __restrict__ rtk, const float* __restrict__ verts, int F,
                                                             int per_frame, long long V, int vp, int turntable, double W, double H,
                                                             double out_width, float* __restrict__ cams, float* __restrict__ ctrajs) {
    __shared__ double s_sum[kWaves][3];
    const int f = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double mean[3] = {0.0, 0.0, 0.0};
    if (vp == 1 || vp == 2) {                                                         // workgroup-uniform
        const float* p = verts + (per_frame ? (long long)f * V * 3 : 0);
        double acc[3] = {0.0, 0.0, 0.0};
        for (long long v = threadIdx.x; v < V; v += kBlock) {
            acc[0] += (double)p[v * 3];
            acc[1] += (double)p[v * 3 + 1];
            acc[2] += (double)p[v * 3 + 2];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double t = wave_add(acc[a]);
            if (lane == 0) s_sum[wave][a] = t;
        }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double t = s_sum[0][a];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) t += s_sum[w][a];
            mean[a] = t / (double)V;
        }
    }
    if (threadIdx.x != 0) return;
    const float* c0 = rtk;
    const float* ci = rtk + (long long)f * 16;
    M3 R0, R;
    double t0[3], t[3], k0[4], k[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            R0.m[i * 3 + j] = (double)c0[i * 4 + j];
            R.m[i * 3 + j] = (double)ci[i * 4 + j];
        }
        t0[i] = (double)c0[i * 4 + 3];
        t[i] = (double)ci[i * 4 + 3];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        k0[j] = (double)c0[12 + j];
        k[j] = (double)ci[12 + j];
    }
    if (turntable) {                                                                  // render_vis.py:267-275
        const double angle = ((double)f * 2.0 * 3.141592653589793) / (double)F;
        R = mul3(rodrigues_axis(1, angle), R0);
        t[0] = 0.0; t[1] = 0.0; t[2] = t0[2];
        k[0] = k0[0]; k[1] = k0[1]; k[2] = W / 2.0; k[3] = H / 2.0;
    }
    M3 Rv = R;
    if (vp == 1 || vp == 2) {                                                         // :309-320
        Rv = mul3(rodrigues_axis(vp == 1 ? 1 : 0, 3.141592653589793 / 2.0), R);
#pragma unroll
        for (int a = 0; a < 2; ++a) t[a] = -((Rv.m[a * 3] * mean[0] + Rv.m[a * 3 + 1] * mean[1]) + Rv.m[a * 3 + 2] * mean[2]);
    } else if (vp == MODA_SEQVIS_VP_STATIC || vp == MODA_SEQVIS_VP_CANONICAL) {       // :290-308
        const M3 lead = vp == MODA_SEQVIS_VP_STATIC
                            ? R0 : mul3(rodrigues_axis(1, 3.141592653589793 / 3.0), rodrigues_axis(0, 3.141592653589793));
        Rv = mul3(mul3(lead, transpose3(R)), R);
        if (vp == MODA_SEQVIS_VP_STATIC) { t[0] = t0[0]; t[1] = t0[1]; }
        else { t[0] = 0.0; t[1] = 0.0; }
        t[2] = t0[2];
        k[0] = k0[0]; k[1] = k0[1];
        k[2] = k0[2] / W * W;
        k[3] = k0[3] / H * H;
    }
    float* o = cams + (long long)f * 16;
    float* q = ctrajs + (long long)f * 16;
    const double scale = out_width / W;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) o[i * 4 + j] = q[i * 4 + j] = (float)Rv.m[i * 3 + j];
        o[i * 4 + 3] = q[i * 4 + 3] = (float)t[i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float kf = (float)k[j];
        o[12 + j] = kf;
        q[12 + j] = (float)((double)kf * scale);
    }
}

// ---- project ------------------------------------------------------------------------------------------------------------------
DEVINL float cam_row(const float* __restrict__ c, int r, float x, float y, float z) {
    return ((c[r * 4] * x + c[r * 4 + 1] * y) + c[r * 4 + 2] * z) + c[r * 4 + 3];
}

__global__ __launch_bounds__(kBlock) void seqvis_project_kernel(const float* __restrict__ verts, const float* __restrict__ cams,
                                                                const int* __restrict__ faces, int n, int per_frame, int V, int Nf,
                                                                int S, unsigned vblocks, unsigned fblocks, float* __restrict__ cam,
                                                                float* __restrict__ ndc, int* __restrict__ view_faces,
                                                                int* __restrict__ status) {
    __shared__ float s_cam[kBlock * 3], s_ndc[kBlock * 3];
    const int view = blockIdx.y;
    const float* c = cams + (long long)view * 16;
    const float* p = verts + (per_frame ? (long long)view * V * 3 : 0);
    if (blockIdx.x < vblocks) {
        const int v0 = blockIdx.x * kBlock, v = v0 + threadIdx.x;
        bool bad = false;
        if (v < V) {
            const float x = p[(long long)v * 3], y = p[(long long)v * 3 + 1], z = p[(long long)v * 3 + 2];
            const float X = cam_row(c, 0, x, y, z), Y = cam_row(c, 1, x, y, z), Z = cam_row(c, 2, x, y, z);
            const float Zs = fabsf(Z) < 1e-12f ? 1e-12f : Z;
            const float u = c[12] * X / Zs + c[14], w = c[13] * Y / Zs + c[15];
            const float sc = (float)(2.0 / (double)S);
            const float nx = u * sc - 1.0f, ny = -(w * sc - 1.0f);
            s_cam[threadIdx.x * 3] = X; s_cam[threadIdx.x * 3 + 1] = Y; s_cam[threadIdx.x * 3 + 2] = Z;
            s_ndc[threadIdx.x * 3] = nx; s_ndc[threadIdx.x * 3 + 1] = ny; s_ndc[threadIdx.x * 3 + 2] = Z;
            bad = !(isfinite(nx) && isfinite(ny) && isfinite(Z));
        }
        wave_count(bad, status + MODA_SEQVIS_NONFINITE);
        __syncthreads();
        const int rows = min(kBlock, V - v0);
        const long long base = ((long long)view * V + v0) * 3;
        for (int i = threadIdx.x; i < rows * 3; i += kBlock) {
            cam[base + i] = s_cam[i];
            ndc[base + i] = s_ndc[i];
        }
        return;
    }
    const int face = (blockIdx.x - vblocks) * kBlock + threadIdx.x;
    bool dropped = false, bad_index = false;
    if (face < Nf) {
        int id[3];
        bool in_range = true, front = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            id[a] = faces[(long long)face * 3 + a];
            in_range = in_range && id[a] >= 0 && id[a] < V;
        }
        if (in_range) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float* q = p + (long long)id[a] * 3;
                front = front && cam_row(c, 2, q[0], q[1], q[2]) > 0.0f;
            }
        }
        bad_index = !in_range;
        dropped = in_range && !front;
        const bool keep = in_range && front;
        int* o = view_faces + ((long long)view * Nf + face) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = keep ? id[a] : -1;
    }
    wave_count(dropped, status + MODA_SEQVIS_DROPPED);
    wave_count(bad_index, status + MODA_SEQVIS_BAD_INDEX);
}

// ---- records ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void seqvis_records_kernel(const float* __restrict__ cam, const int* __restrict__ view_faces,
                                                                const int* __restrict__ csr_off, const int* __restrict__ csr_ent,
                                                                int V, int Nf, int mode, const uint8_t* __restrict__ colors,
                                                                int colors_per_frame, float color_const,
                                                                const float* __restrict__ error, const float* __restrict__ table,
                                                                float* __restrict__ rec, int* __restrict__ status) {
    const int view = blockIdx.y, v = blockIdx.x * kBlock + threadIdx.x;
    bool nan_error = false;
    if (v < V) {
        const float* pv = cam + (long long)view * V * 3;
        const int* vf = view_faces + (long long)view * Nf * 3;
        float nx = 0.f, ny = 0.f, nz = 0.f;
        const int e1 = csr_off[v + 1];
        for (int e = csr_off[v]; e < e1; ++e) {
            const int face = csr_ent[e] / 3;
            if (face < 0 || face >= Nf) continue;
            const int i0 = vf[face * 3], i1 = vf[face * 3 + 1], i2 = vf[face * 3 + 2];
            if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) continue;
            const float* a = pv + (long long)i0 * 3;
            const float* b = pv + (long long)i1 * 3;
            const float* c = pv + (long long)i2 * 3;
            const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2];
            const float wx = c[0] - a[0], wy = c[1] - a[1], wz = c[2] - a[2];
            nx += uy * wz - uz * wy;
            ny += uz * wx - ux * wz;
            nz += ux * wy - uy * wx;
        }
        const float len = fmaxf(sqrtf((nx * nx + ny * ny) + nz * nz), 1e-12f);
        float r, g, b;
        if (mode == MODA_SEQVIS_COLOR_U8) {
            const uint8_t* q = colors + ((colors_per_frame ? (long long)view * V : 0) + v) * 3;
            r = (float)((3 * (int)q[0]) / 5);
            g = (float)((3 * (int)q[1]) / 5);
            b = (float)((3 * (int)q[2]) / 5);
        } else if (mode == MODA_SEQVIS_COLOR_ERROR) {
            const float x = 5.0f * error[(long long)view * V + v];
            nan_error = x != x;
            int idx = x < 0.f ? 0 : (x >= 1.f ? 255 : (int)(x * 256.0f));
            idx = min(max(idx, 0), 255);
            r = nan_error ? 0.f : table[idx * 3];
            g = nan_error ? 0.f : table[idx * 3 + 1];
            b = nan_error ? 0.f : table[idx * 3 + 2];
        } else {
            r = g = b = color_const;
        }
        float4* o = reinterpret_cast<float4*>(rec + ((long long)view * V + v) * kRec);
        o[0] = make_float4(r, g, b, nx / len);
        o[1] = make_float4(ny / len, nz / len, 0.f, 0.f);
    }
    wave_count(nan_error, status + MODA_SEQVIS_NAN_ERROR);
}

// ---- shade --------------------------------------------------------------------------------------------------------------------
struct Layer { bool on; float rgb[3]; float z; };

DEVINL Layer shade_layer(const int* __restrict__ face_idx, const float* __restrict__ bary, const float* __restrict__ zbuf,
                         const int* __restrict__ faces, const float* __restrict__ rec, const float* __restrict__ cam, int V, int Nf,
                         long long pix, long long view, int smooth) {
    Layer L;
    L.on = false;
    L.rgb[0] = L.rgb[1] = L.rgb[2] = 0.f;
    L.z = 0.f;
    const int face = face_idx[pix];
    if (face < 0 || face >= Nf) return L;
    const int i0 = faces[face * 3], i1 = faces[face * 3 + 1], i2 = faces[face * 3 + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return L;
    const float b0 = bary[pix * 3], b1 = bary[pix * 3 + 1], b2 = bary[pix * 3 + 2];
    const float4* r0 = reinterpret_cast<const float4*>(rec + (view * V + i0) * kRec);
    const float4* r1 = reinterpret_cast<const float4*>(rec + (view * V + i1) * kRec);
    const float4* r2 = reinterpret_cast<const float4*>(rec + (view * V + i2) * kRec);
    const float4 a0 = r0[0], a1 = r1[0], a2 = r2[0];
    float nx, ny, nz;
    if (smooth) {
        const float4 c0 = r0[1], c1 = r1[1], c2 = r2[1];
        nx = (b0 * a0.w + b1 * a1.w) + b2 * a2.w;
        ny = (b0 * c0.x + b1 * c1.x) + b2 * c2.x;
        nz = (b0 * c0.y + b1 * c1.y) + b2 * c2.y;
    } else {
        const float* p0 = cam + (view * V + i0) * 3;
        const float* p1 = cam + (view * V + i1) * 3;
        const float* p2 = cam + (view * V + i2) * 3;
        const float ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
        const float wx = p2[0] - p0[0], wy = p2[1] - p0[1], wz = p2[2] - p0[2];
        nx = uy * wz - uz * wy;
        ny = uz * wx - ux * wz;
        nz = ux * wy - uy * wx;
    }
    const float lambert = fabsf(nz) / fmaxf(sqrtf((nx * nx + ny * ny) + nz * nz), 1e-12f);
    const float k = 0.4f + lambert;
    L.rgb[0] = fminf(fmaxf(((b0 * a0.x + b1 * a1.x) + b2 * a2.x) * k, 0.f), 255.f);
    L.rgb[1] = fminf(fmaxf(((b0 * a0.y + b1 * a1.y) + b2 * a2.y) * k, 0.f), 255.f);
    L.rgb[2] = fminf(fmaxf(((b0 * a0.z + b1 * a1.z) + b2 * a2.z) * k, 0.f), 255.f);
    L.z = zbuf[pix];
    L.on = true;
    return L;
}

__global__ __launch_bounds__(kBlock) void seqvis_shade_kernel(
    const int* __restrict__ face_idx, const float* __restrict__ bary, const float* __restrict__ zbuf, const int* __restrict__ faces,
    const float* __restrict__ rec, const float* __restrict__ cam, int V, int Nf, const int* __restrict__ face_idx_b,
    const float* __restrict__ bary_b, const float* __restrict__ zbuf_b, const int* __restrict__ faces_b,
    const float* __restrict__ rec_b, const float* __restrict__ cam_b, int Vb, int Nfb, int S, int H, int W, int smooth, float opacity,
    const uint8_t* __restrict__ overlay, uint8_t* __restrict__ color, float* __restrict__ depth, int16_t* __restrict__ sil,
    int* __restrict__ sil_count) {
    const long long view = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;                                 // pixel of the H x W window, row major
    bool covered = false;
    if (i < H * W) {
        const int row = i / W, col = i - row * W;
        const long long pix = (view * S + row) * S + col;
        const Layer body = shade_layer(face_idx, bary, zbuf, faces, rec, cam, V, Nf, pix, view, smooth);
        Layer bone;
        bone.on = false;
        if (face_idx_b) bone = shade_layer(face_idx_b, bary_b, zbuf_b, faces_b, rec_b, cam_b, Vb, Nfb, pix, view, smooth);
        float out[3] = {0.f, 0.f, 0.f}, z = 0.f;
        if (body.on && bone.on) {
            const bool front = bone.z < body.z;
            z = front ? bone.z : body.z;
#pragma unroll
            for (int a = 0; a < 3; ++a) out[a] = front ? bone.rgb[a] : opacity * body.rgb[a] + (1.0f - opacity) * bone.rgb[a];
        } else if (body.on || bone.on) {
            const Layer& l = body.on ? body : bone;
            z = l.z;
#pragma unroll
            for (int a = 0; a < 3; ++a) out[a] = l.rgb[a];
        }
        const long long o = view * H * W + i;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int c = (int)fminf(fmaxf(out[a], 0.f), 255.f);
            if (overlay) {
                const int s = c + (int)overlay[o * 3 + a];
                c = s >> 1;
                if (s & 1) c += c & 1;
            }
            color[o * 3 + a] = (uint8_t)(i == 0 ? 0 : c);
        }
        depth[o] = z;
        covered = z > 0.f;
        sil[o] = covered ? (int16_t)100 : (int16_t)0;
    }
    wave_count(covered, sil_count + view);
}

// ---- resize -------------------------------------------------------------------------------------------------------------------
DEVINL void axis_taps(int d, float scale, int n, int* i0, int* i1, float* w1) {
    const float s = ((float)d + 0.5f) * scale - 0.5f;
    const float fl = floorf(s);
    const int a = (int)fl;
    *w1 = s - fl;
    *i0 = min(max(a, 0), n - 1);
    *i1 = min(max(a + 1, 0), n - 1);
}

__global__ __launch_bounds__(kBlock) void seqvis_resize_kernel(const uint8_t* __restrict__ color, const int16_t* __restrict__ sil,
                                                               const int* __restrict__ sil_count, int H, int W, int h, int w,
                                                               float sy, float sx, uint8_t* __restrict__ frames,
                                                               int16_t* __restrict__ refsil, int* __restrict__ status) {
    const long long view = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0 && sil_count[view] == 0) atomicAdd(status + MODA_SEQVIS_EMPTY, 1);
    if (i >= h * w) return;
    const int row = i / w, col = i - row * w;
    int y0, y1, x0, x1;
    float wy, wx;
    axis_taps(row, sy, H, &y0, &y1, &wy);
    axis_taps(col, sx, W, &x0, &x1, &wx);
    const long long base = view * H * W;
    const long long p00 = base + (long long)y0 * W + x0, p01 = base + (long long)y0 * W + x1;
    const long long p10 = base + (long long)y1 * W + x0, p11 = base + (long long)y1 * W + x1;
    const float w00 = (1.0f - wy) * (1.0f - wx), w01 = (1.0f - wy) * wx, w10 = wy * (1.0f - wx), w11 = wy * wx;
    const long long o = view * h * w + i;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float v = ((w00 * (float)color[p00 * 3 + a] + w01 * (float)color[p01 * 3 + a]) + w10 * (float)color[p10 * 3 + a])
                        + w11 * (float)color[p11 * 3 + a];
        frames[o * 3 + a] = (uint8_t)fminf(fmaxf(rintf(v), 0.f), 255.f);
    }
    const float v = ((w00 * (float)sil[p00] + w01 * (float)sil[p01]) + w10 * (float)sil[p10]) + w11 * (float)sil[p11];
    refsil[o] = (int16_t)rintf(v);
}

inline bool frames_ok(int64_t n, int64_t Fv) { return Fv == 1 || Fv == n; }

}   // namespace

extern "C" int moda_seqvis_cams(const float* rtk, const float* verts, int64_t F, int64_t Fv, int64_t V, int32_t vp, int32_t turntable,
                                int64_t W, int64_t H, int64_t out_width, float* cams, float* ctrajs, void* stream) {
    if (F < 1 || F > (1 << 24) || V < 1 || V >= 0x7fffffffLL || !frames_ok(F, Fv) || W < 1 || H < 1 || out_width < 1 || vp < -2 || vp > 2)
        return MODA_ESHAPE;
    if (!rtk || !verts || !cams || !ctrajs) return MODA_EINVAL;
    hipLaunchKernelGGL(seqvis_cams_kernel, dim3((unsigned)F), dim3(kBlock), 0, (hipStream_t)stream, rtk, verts, (int)F, (int)(Fv == F && F > 1),
                       (long long)V, (int)vp, (int)turntable, (double)W, (double)H, (double)out_width, cams, ctrajs);
    return (int)hipGetLastError();
}

extern "C" int moda_seqvis_project(const float* verts, const float* cams, const int32_t* faces, int64_t n, int64_t Fv, int64_t V,
                                   int64_t Nf, int64_t S, float* cam, float* ndc, int32_t* view_faces, int32_t* status, void* stream) {
    if (n < 1 || V < 1 || Nf < 1 || S < 1 || S > 32768 || n > 65535 || n * V >= 0x7fffffffLL / 3 || n * Nf >= 0x7fffffffLL / 3
        || !frames_ok(n, Fv))
        return MODA_ESHAPE;
    if (!verts || !cams || !faces || !cam || !ndc || !view_faces || !status) return MODA_EINVAL;
    const unsigned vb = nblocks(V, kBlock), fb = nblocks(Nf, kBlock);
    hipLaunchKernelGGL(seqvis_project_kernel, dim3(vb + fb, (unsigned)n), dim3(kBlock), 0, (hipStream_t)stream, verts, cams, faces, (int)n,
                       (int)(Fv == n && n > 1), (int)V, (int)Nf, (int)S, vb, fb, cam, ndc, view_faces, status);
    return (int)hipGetLastError();
}

extern "C" int moda_seqvis_records(const float* cam, const int32_t* view_faces, const int32_t* csr_off, const int32_t* csr_ent,
                                   int64_t n, int64_t V, int64_t Nf, int32_t color_mode, const uint8_t* colors_u8, int64_t Fc,
                                   float color_const, const float* error, const float* table, float* rec, int32_t* status,
                                   void* stream) {
    if (n < 1 || V < 1 || Nf < 1 || n > 65535 || n * V >= (1LL << 28) || n * Nf >= 0x7fffffffLL / 3 || !frames_ok(n, Fc)) return MODA_ESHAPE;
    if (!cam || !view_faces || !csr_off || !csr_ent || !rec || !status || (((uintptr_t)rec) & 31)) return MODA_EINVAL;
    if (color_mode == MODA_SEQVIS_COLOR_U8 ? !colors_u8 : color_mode == MODA_SEQVIS_COLOR_ERROR ? (!error || !table)
                                                                                                 : color_mode != MODA_SEQVIS_COLOR_CONST)
        return MODA_EINVAL;
    hipLaunchKernelGGL(seqvis_records_kernel, dim3(nblocks(V, kBlock), (unsigned)n), dim3(kBlock), 0, (hipStream_t)stream, cam, view_faces,
                       csr_off, csr_ent, (int)V, (int)Nf, (int)color_mode, colors_u8, (int)(Fc == n && n > 1), color_const, error, table,
                       rec, status);
    return (int)hipGetLastError();
}

extern "C" int moda_seqvis_shade(const int32_t* face_idx, const float* bary, const float* zbuf, const int32_t* faces, const float* rec,
                                 const float* cam, int64_t V, int64_t Nf, const int32_t* face_idx_b, const float* bary_b,
                                 const float* zbuf_b, const int32_t* faces_b, const float* rec_b, const float* cam_b, int64_t Vb,
                                 int64_t Nfb, int64_t n, int64_t S, int64_t H, int64_t W, int32_t smooth, float opacity,
                                 const uint8_t* overlay, uint8_t* color, float* depth, void* sil, int32_t* sil_count, void* stream) {
    if (n < 1 || n > 65535 || H < 1 || W < 1 || H > S || W > S || S > 32768 || n * S * S >= 0x7fffffffLL || V < 1 || Nf < 1
        || n * V >= (1LL << 28) || Nf >= 0x7fffffffLL / 3)
        return MODA_ESHAPE;
    if (!face_idx || !bary || !zbuf || !faces || !rec || !cam || !color || !depth || !sil || !sil_count || (((uintptr_t)rec) & 31))
        return MODA_EINVAL;
    if (face_idx_b) {
        if (Vb < 1 || Nfb < 1 || n * Vb >= (1LL << 28) || Nfb >= 0x7fffffffLL / 3) return MODA_ESHAPE;
        if (!bary_b || !zbuf_b || !faces_b || !rec_b || !cam_b || (((uintptr_t)rec_b) & 31)) return MODA_EINVAL;
    }
    hipLaunchKernelGGL(seqvis_shade_kernel, dim3(nblocks(H * W, kBlock), (unsigned)n), dim3(kBlock), 0, (hipStream_t)stream, face_idx, bary,
                       zbuf, faces, rec, cam, (int)V, (int)Nf, face_idx_b, bary_b, zbuf_b, faces_b, rec_b, cam_b, (int)Vb, (int)Nfb,
                       (int)S, (int)H, (int)W, (int)smooth, opacity, overlay, color, depth, (int16_t*)sil, sil_count);
    return (int)hipGetLastError();
}

extern "C" int moda_seqvis_resize(const uint8_t* color, const void* sil, const int32_t* sil_count, int64_t n, int64_t H, int64_t W,
                                  int64_t h, int64_t w, uint8_t* frames, void* refsil, int32_t* status, void* stream) {
    if (n < 1 || n > 65535 || H < 1 || W < 1 || h < 1 || w < 1 || H > 32768 || W > 32768 || h > 32768 || w > 32768
        || n * H * W >= 0x7fffffffLL / 3 || n * h * w >= 0x7fffffffLL / 3)
        return MODA_ESHAPE;
    if (!color || !sil || !sil_count || !frames || !refsil || !status) return MODA_EINVAL;
    hipLaunchKernelGGL(seqvis_resize_kernel, dim3(nblocks(h * w, kBlock), (unsigned)n), dim3(kBlock), 0, (hipStream_t)stream, color,
                       (const int16_t*)sil, sil_count, (int)H, (int)W, (int)h, (int)w, (float)((double)H / (double)h),
                       (float)((double)W / (double)w), frames, (int16_t*)refsil, status);
    return (int)hipGetLastError();
}
