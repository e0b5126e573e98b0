// shm/temporal.h — the temporal pass's arithmetic: the frame just rendered is blended into a per-pixel history that the G-buffer's render-space position carries from the
// previous frame's camera to this one's (the reprojection and the history length of SVGF, Schied et al. 2017, without its feedback of the filtered colour), on the
// denoiser's albedo-demodulated radiance.
// Single source like every header here: k_temporal.hip compiles it for the device, host/host_mirror.cpp for the CPU twin (shm_temporal_accumulate_host), and the two are
// held to each other bit for bit (tests/test_gpu_temporal.py). Only correctly rounded operations: no contraction, no fast-math.
//
// The definition is DESIGN.md section 4l. In short, per pixel (x, y) of a width x height film (pixel_bounds' own coordinates):
//   prepare    c, the guide's validity, a_eff, c' = c / a_eff, l, P and N: denoise_prepare_pixel (shm/denoise.h), unchanged. No usable guide: the result is c, the record empty.
//   motion     m = raster_prev(P) - raster_cur(P), raster_k(P) = raster_from_camera_k (camera_from_render_k P) with the w-divide: a still camera gives m = 0 exactly
//   taps       the four bilinear taps around (x + 0.5 + m.x, y + 0.5 + m.y), row-major; one counts iff it is inside the film, its weight is above 0, its record has a
//              history, dot(N, N_tap) >= normal_cos_min and |dot(N, P_tap - P)| <= plane_tolerance * scale; h = their weighted mean (sums from +0, in that order)
//   blend      length = min(h.length + 1, max_history), a = max(1 / length, alpha_min), rgb = h.rgb + a (c' - h.rgb), the two moments of l alike; no tap: length 1, rgb = c'
//   finish     out = rgb a_eff (denoise_finish_pixel)
// Every index a tap is loaded from was clamped into the film first, and a motion that is not finite, or leads off the film, never becomes an index.
#pragma once
#include "denoise.h"

namespace shm {

// ShmTemporalParams (include/shimmer_hip.h) as the kernel takes it
struct TemporalConfig {
    Float alpha_min, alpha_min_moments, max_history, normal_cos_min, plane_tolerance, albedo_floor;
    uint32_t demodulate;
};
// One camera as the pass projects through it: raster_from_camera is the inverse of ShmCamera::camera_from_raster, taken once on the host in double and rounded
struct TemporalCamera {
    Float raster_from_camera[16], camera_from_render[16];
    uint32_t perspective;  // 0: orthographic
};
// ShmTemporalPixel as four 16-byte words: a = (rgb, m1), b = (m2, length, p.xy), c = (p.z, ns), d = the pad
struct alignas(16) TemporalRecord { DnF4 a, b, c, d; };

constexpr Float TEMPORAL_VARIANCE_MIN_LENGTH = 4.0f;  // SVGF: the temporal variance is taken where the history holds four frames or more

// nullptr, or what is wrong with the parameters (shm_temporal_accumulate_device and shm_temporal_accumulate_host refuse them with this message)
inline const char* temporal_params_error(const TemporalConfig& k) {
    if (!(k.alpha_min >= 0.0f && k.alpha_min <= 1.0f)) return "temporal: alpha_min outside [0, 1]";
    if (!(k.alpha_min_moments >= 0.0f && k.alpha_min_moments <= 1.0f)) return "temporal: alpha_min_moments outside [0, 1]";
    if (!(k.max_history >= 1.0f)) return "temporal: max_history is NaN or below 1";
    if (!(k.normal_cos_min >= -1.0f && k.normal_cos_min <= 1.0f)) return "temporal: normal_cos_min outside [-1, 1]";
    if (!(k.plane_tolerance > 0.0f)) return "temporal: plane_tolerance is NaN or not above 0";
    if (!(k.albedo_floor > 0.0f && k.albedo_floor <= 1.0f)) return "temporal: albedo_floor outside (0, 1]";
    return nullptr;
}

// A ShmCamera's two matrices as the pass takes them (host only): camera_from_raster inverted by Gauss-Jordan elimination with partial pivoting, in double, each entry
// rounded to float once. False for a singular matrix. cfr, cfrender: ShmCamera::camera_from_raster and ::camera_from_render.
inline bool temporal_camera(const float* cfr, const float* cfrender, bool perspective, TemporalCamera& out) {
    double a[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { a[i][j] = (double)cfr[i * 4 + j]; a[i][4 + j] = i == j ? 1.0 : 0.0; }
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int i = col + 1; i < 4; ++i)
            if (__builtin_fabs(a[i][col]) > __builtin_fabs(a[piv][col])) piv = i;
        if (!(__builtin_fabs(a[piv][col]) > 0.0)) return false;
        for (int j = 0; j < 8; ++j) { const double t = a[col][j]; a[col][j] = a[piv][j]; a[piv][j] = t; }
        const double d = a[col][col];
        for (int j = 0; j < 8; ++j) a[col][j] /= d;
        for (int i = 0; i < 4; ++i) {
            if (i == col) continue;
            const double f = a[i][col];
            for (int j = 0; j < 8; ++j) a[i][j] -= f * a[col][j];
        }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            out.raster_from_camera[i * 4 + j] = (float)a[i][4 + j];
            out.camera_from_render[i * 4 + j] = cfrender[i * 4 + j];
        }
    out.perspective = perspective ? 1u : 0u;
    return true;
}

SHM_HD TemporalRecord temporal_empty_record() {
    TemporalRecord r;
    r.a = dn_f4(0.0f, 0.0f, 0.0f, 0.0f); r.b = r.a; r.c = r.a; r.d = r.a;
    return r;
}

// raster_from_camera (camera_from_render P): the raster point and the depth along the camera's axis. False where the point has no image: at or behind a perspective
// camera, or with a w that is not above 0.
SHM_HD bool temporal_raster(const TemporalCamera& k, const Float* P, Float& rx, Float& ry, Float& depth) {
    const Float* m = k.camera_from_render;
    const Float cx = ((m[0] * P[0] + m[1] * P[1]) + m[2] * P[2]) + m[3];
    const Float cy = ((m[4] * P[0] + m[5] * P[1]) + m[6] * P[2]) + m[7];
    const Float cz = ((m[8] * P[0] + m[9] * P[1]) + m[10] * P[2]) + m[11];
    depth = cz;
    if (k.perspective && !(cz > 0.0f)) return false;
    const Float* r = k.raster_from_camera;
    const Float xr = ((r[0] * cx + r[1] * cy) + r[2] * cz) + r[3];
    const Float yr = ((r[4] * cx + r[5] * cy) + r[6] * cz) + r[7];
    const Float wr = ((r[12] * cx + r[13] * cy) + r[14] * cz) + r[15];
    if (!(wr > 0.0f)) return false;
    rx = xr / wr;
    ry = yr / wr;
    return true;
}

// The history of a valid pixel: h = (rgb, m1 | m2, length) as the weighted mean of the taps that count; false where none does. N, P: the pixel's own; `history`: the
// previous frame's records, width x height.
SHM_HD bool temporal_gather(const TemporalRecord* history, const TemporalCamera& cur, const TemporalCamera& prev, int x, int y, int width, int height, const Float* N,
                            const Float* P, const TemporalConfig& k, DnF4& h_a, Float& h_m2, Float& h_length) {
    Float cx, cy, cd, px, py, pd;
    if (!temporal_raster(cur, P, cx, cy, cd) || !temporal_raster(prev, P, px, py, pd)) return false;
    const Float mx = px - cx, my = py - cy;
    if (!is_finite(mx) || !is_finite(my)) return false;
    // the history position less the half pixel of a pixel's centre: the taps' own coordinates
    const Float fx = (((Float)x + 0.5f) + mx) - 0.5f, fy = (((Float)y + 0.5f) + my) - 0.5f;
    if (!(fx > -1.0f && fx < (Float)width && fy > -1.0f && fy < (Float)height)) return false;  // (all four taps outside; a NaN ends here too)
    const Float x0f = floor(fx), y0f = floor(fy);
    const Float tx = fx - x0f, ty = fy - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;  // in [-1, width - 1] x [-1, height - 1]
    const Float scale = prev.perspective ? pd : 1.0f;
    const Float limit = k.plane_tolerance * scale;
    Float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, s1 = 0.0f, s2 = 0.0f, sl = 0.0f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int qx = x0 + i, qy = y0 + j;
            const bool inside = qx >= 0 && qy >= 0 && qx < width && qy < height;
            const Float w = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
            if (!inside || !(w > 0.0f)) continue;
            // (inside: the clamp changes nothing; it is what makes the address one of the film's whatever the branch above becomes)
            const int ux = qx < 0 ? 0 : (qx >= width ? width - 1 : qx), uy = qy < 0 ? 0 : (qy >= height ? height - 1 : qy);
            const TemporalRecord* t = history + ((size_t)uy * (size_t)width + (size_t)ux);
            const DnF4 tb = t->b;
            if (!(tb.y > 0.0f)) continue;  // no history there
            const DnF4 tc = t->c;
            const Float dn = (N[0] * tc.y + N[1] * tc.z) + N[2] * tc.w;
            if (!(dn >= k.normal_cos_min)) continue;
            const Float dx = tb.z - P[0], dy = tb.w - P[1], dz = tc.x - P[2];
            const Float off = abs((N[0] * dx + N[1] * dy) + N[2] * dz);
            if (!(off <= limit)) continue;
            const DnF4 ta = t->a;
            sw += w;
            sr += w * ta.x;
            sg += w * ta.y;
            sb += w * ta.z;
            s1 += w * ta.w;
            s2 += w * tb.x;
            sl += w * tb.y;
        }
    if (!(sw > 0.0f)) return false;
    h_a = dn_f4(sr / sw, sg / sw, sb / sw, s1 / sw);
    h_m2 = s2 / sw;
    h_length = sl / sw;
    return true;
}

// One pixel: the record to keep and the result (a ShmFilmPixel's 4 doubles). film, g, white: as denoise_prepare_pixel takes them; `history` null: no previous frame (then
// `prev` is not read).
SHM_HD void temporal_pixel(const double* film, const double* g, const Float* white, const TemporalRecord* history, const TemporalCamera& cur, const TemporalCamera& prev,
                           int x, int y, int width, int height, const TemporalConfig& k, TemporalRecord& rec, double* out) {
    const DenoiseConfig dk{0u, k.demodulate, 1.0f, 1.0f, 1.0f, k.albedo_floor};  // (prepare reads demodulate and albedo_floor only)
    DnF4 A, B, C, D;
    denoise_prepare_pixel(film, g, white, dk, A, B, C, D);
    rec = temporal_empty_record();
    if (C.w == 0.0f) {  // pass-through: c, bit for bit, and no history starts here
        denoise_finish_pixel(film, false, A, D, out);
        return;
    }
    const Float N[3] = {B.x, B.y, B.z}, P[3] = {C.x, C.y, C.z};
    const Float l = B.w;  // denoise_luminance(c')
    DnF4 h_a;
    Float h_m2 = 0.0f, h_length = 0.0f;
    DnF4 r = dn_f4(A.x, A.y, A.z, l);
    Float m2 = l * l, length = 1.0f;
    if (history && temporal_gather(history, cur, prev, x, y, width, height, N, P, k, h_a, h_m2, h_length)) {
        length = min(h_length + 1.0f, k.max_history);
        const Float inv = 1.0f / length;
        const Float a = max(inv, k.alpha_min), am = max(inv, k.alpha_min_moments);
        r.x = h_a.x + a * (A.x - h_a.x);
        r.y = h_a.y + a * (A.y - h_a.y);
        r.z = h_a.z + a * (A.z - h_a.z);
        r.w = h_a.w + am * (l - h_a.w);
        m2 = h_m2 + am * (l * l - h_m2);
    }
    rec.a = r;
    rec.b = dn_f4(m2, length, P[0], P[1]);
    rec.c = dn_f4(P[2], N[0], N[1], N[2]);
    denoise_finish_pixel(film, true, r, D, out);
}

// The a-trous filter's initial variance from a record (shm_denoise_temporal_*, temporal_variance = 1): max(0, m2 - m1^2) / length
SHM_HD Float temporal_variance(const TemporalRecord& t) {
    const Float v = t.b.x - t.a.w * t.a.w;
    return (v > 0.0f ? v : 0.0f) / t.b.y;
}

}  // namespace shm
