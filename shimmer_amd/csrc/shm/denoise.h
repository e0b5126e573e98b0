// shm/denoise.h — the denoiser's arithmetic: a single-frame, edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with SVGF's weights and its spatial variance
// estimate (Schied et al. 2017), on albedo-demodulated radiance, guided by the G-buffer pass's shading normal, position, albedo and coverage.
// Single source like every header here: k_denoise.hip compiles it for the device, host/host_mirror.cpp for the CPU twin (shm_denoise_host), and the two are held to each
// other bit for bit (tests/test_gpu_denoise.py). Only correctly rounded operations and fp.h's exp / log (which are built from such operations, explicit fma among them): no contraction, no fast-math.
//
// The definition is DESIGN.md section 4j; a float64 restatement can be written from that text alone (tests/test_denoise.py holds one). In short, per pixel:
//   prepare    c, the guides, validity, a_eff and e = c / a_eff from the film's and the G-buffer's double sums      -> planes A (e.rgb, var), B (n.xyz, l), C (p.xyz, valid), D (a_eff)
//   variance   var = max(0, m2 - m1^2) of l over a 7x7 window, weighted by w_n w_z                                  -> A.w
//   a-trous    iteration i: the 5x5 B3 spline, taps 2^i apart, w = h w_n w_z w_l; e' = sum w e / sum w, var' = sum w^2 var / (sum w)^2   A -> A'
//   finish     out = e a_eff for a valid pixel, c for a pass-through one
// Every window is walked row-major (dy outer, dx inner, both increasing) and every sum starts at +0 and adds in that order; a tap outside the film or on a pass-through
// pixel is skipped: nothing is added for it.
#pragma once
#include "fp.h"
#include "moments.h"  // the measured variance (denoise_measured_variance, at the end)

namespace shm {

struct alignas(16) DnF4 { Float x, y, z, w; };

// ShmDenoiseParams (include/shimmer_hip.h) as the kernels take it
struct DenoiseConfig {
    uint32_t iterations, demodulate;
    Float sigma_luminance, sigma_normal, sigma_plane, albedo_floor;
};

constexpr Float DENOISE_TINY = 1e-10f;         // added to both exponents' denominators
constexpr uint32_t DENOISE_MAX_ITERATIONS = 8;

SHM_HD DnF4 dn_f4(Float x, Float y, Float z, Float w) { DnF4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }
// l: the mean of e's three channels
SHM_HD Float denoise_luminance(const DnF4& e) { return ((e.x + e.y) + e.z) / 3.0f; }

// nullptr, or what is wrong with the parameters (shm_denoise_device and shm_denoise_host refuse them with this message)
inline const char* denoise_params_error(const DenoiseConfig& k) {
    if (k.iterations > DENOISE_MAX_ITERATIONS) return "denoise: iterations above 8";
    if (!(k.sigma_luminance > 0.0f)) return "denoise: sigma_luminance is NaN or not above 0";
    if (!(k.sigma_normal > 0.0f)) return "denoise: sigma_normal is NaN or not above 0";
    if (!(k.sigma_plane > 0.0f)) return "denoise: sigma_plane is NaN or not above 0";
    if (!(k.albedo_floor > 0.0f && k.albedo_floor <= 1.0f)) return "denoise: albedo_floor outside (0, 1]";
    return nullptr;
}

// c of a pixel: the division shm_film_get_image does (float by float), 0 where weight_sum is 0. film: rgb_sum[3], weight_sum.
SHM_HD void denoise_pixel_colour(const double* film, Float* c) {
    const double weight_sum = film[3];
    if (weight_sum == 0.0) { c[0] = c[1] = c[2] = 0.0f; return; }
    const Float w = (Float)weight_sum;
    for (int k = 0; k < 3; ++k) c[k] = (Float)film[k] / w;
}

// One pixel's planes from its sums. film: a ShmFilmPixel's 4 doubles; g: a ShmGBufferPixel's 16 doubles (p 0, n 3, ns 6, uv 9, albedo 11, weight_hit 14, weight_sum 15);
// white: shm_gbuffer_white's W, rounded to float. A pass-through pixel gets zeros, valid = 0 and a_eff = 1.
SHM_HD void denoise_prepare_pixel(const double* film, const double* g, const Float* white, const DenoiseConfig& k, DnF4& A, DnF4& B, DnF4& C, DnF4& D) {
    A = dn_f4(0.0f, 0.0f, 0.0f, 0.0f); B = A; C = A;
    D = dn_f4(1.0f, 1.0f, 1.0f, 0.0f);
    Float c[3];
    denoise_pixel_colour(film, c);
    const double weight_sum = film[3], weight_hit = g[14];
    if (!(weight_sum > 0.0) || !(weight_hit > 0.0)) return;
    // the coverage is the G-buffer's own ratio: its pass need not have run the samples the render ran
    const Float wh = (Float)weight_hit;
    const Float cov = clamp(wh / (Float)g[15], 0.0f, 1.0f);
    Float ns[3], p[3], a_eff[3], e[3];
    for (int i = 0; i < 3; ++i) {
        ns[i] = (Float)g[6 + i] / wh;
        p[i] = (Float)g[i] / wh;
        const Float a = ((Float)g[11 + i] / wh) / white[i];
        a_eff[i] = 1.0f;
        if (k.demodulate) {
            a_eff[i] = cov * a + (1.0f - cov);
            // below the floor the channel is not demodulated: what a black surface shows is emitted, not reflected, light (an emitter's material is often black), and
            // dividing it by a small albedo would hand it to the neighbours multiplied (a NaN stays one: the pixel passes through)
            if (a_eff[i] < k.albedo_floor) a_eff[i] = 1.0f;
        }
        e[i] = c[i] / a_eff[i];
    }
    const Float len = sqrt((ns[0] * ns[0] + ns[1] * ns[1]) + ns[2] * ns[2]);
    if (!(len > 0.0f)) return;
    Float n[3];
    bool finite = true;
    for (int i = 0; i < 3; ++i) {
        n[i] = ns[i] / len;
        finite = finite && is_finite(c[i]) && is_finite(n[i]) && is_finite(p[i]) && is_finite(a_eff[i]) && is_finite(e[i]);
    }
    if (!finite) return;
    A = dn_f4(e[0], e[1], e[2], 0.0f);
    B = dn_f4(n[0], n[1], n[2], denoise_luminance(A));
    C = dn_f4(p[0], p[1], p[2], 1.0f);
    D = dn_f4(a_eff[0], a_eff[1], a_eff[2], 0.0f);
}

// w_n w_z of tap q seen from pixel p (both valid, q != p): 0 where the normals are a right angle or more apart.
//   w_n = max(0, n_p . n_q)^sigma_normal, as exp(sigma_normal log(n_p . n_q))
//   w_z = exp(-|n_p . (p_q - p_p)| / (sigma_plane |p_q - p_p| + tiny)): the sine of the angle the step to q leaves p's tangent plane by, so no scene scale enters
SHM_HD Float denoise_geometry_weight(const DnF4& Bp, const DnF4& Cp, const DnF4& Bq, const DnF4& Cq, const DenoiseConfig& k) {
    const Float d = (Bp.x * Bq.x + Bp.y * Bq.y) + Bp.z * Bq.z;
    if (!(d > 0.0f)) return 0.0f;
    const Float w_n = exp(k.sigma_normal * log(d));
    const Float dx = Cq.x - Cp.x, dy = Cq.y - Cp.y, dz = Cq.z - Cp.z;
    const Float off = abs((Bp.x * dx + Bp.y * dy) + Bp.z * dz);
    const Float dist = sqrt((dx * dx + dy * dy) + dz * dz);
    const Float w_z = exp(-(off / (k.sigma_plane * dist + DENOISE_TINY)));
    return w_n * w_z;
}

// The planes a pixel function reads, as a window around its pixel: tap(i, j, A, B, C) gives the pixel (i, j) taps — `step` pixels each — away and says whether there is one to take —
// false outside the film and on a pass-through pixel. B.w is the tap's l. guides(i, j, B, C) is the same without plane A (the variance pass, which writes A.w). DenoiseGlobalTaps reads the planes where they lie (the CPU twin, k_denoise_variance);
// k_denoise.hip has a second one over the a-trous kernel's LDS tile.
struct DenoiseGlobalTaps {
    const DnF4 *A, *B, *C;
    int x, y, width, height, step;
    bool current_l;  // B.w = denoise_luminance(A) instead of plane B's (the a-trous iterations: plane A moves on, plane B stays)
    SHM_HD bool tap(int i, int j, DnF4& a, DnF4& b, DnF4& c) const {
        const int qx = x + i * step, qy = y + j * step;
        if (qx < 0 || qy < 0 || qx >= width || qy >= height) return false;
        const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
        c = C[q];
        if (c.w == 0.0f) return false;
        a = A[q];
        b = B[q];
        if (current_l) b.w = denoise_luminance(a);
        return true;
    }
    SHM_HD bool guides(int i, int j, DnF4& b, DnF4& c) const {
        const int qx = x + i * step, qy = y + j * step;
        if (qx < 0 || qy < 0 || qx >= width || qy >= height) return false;
        const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
        c = C[q];
        if (c.w == 0.0f) return false;
        b = B[q];
        return true;
    }
};

// h = h1 (x) h1: (1, 4, 6, 4, 1) (x) (1, 4, 6, 4, 1) / 256, and g = g1 (x) g1: (1, 2, 1) (x) (1, 2, 1) / 16 — every entry exact
SHM_HD Float denoise_h1(int i) { return i == 0 ? 0.375f : ((i == 1 || i == -1) ? 0.25f : 0.0625f); }
SHM_HD Float denoise_g1(int i) { return i == 0 ? 0.5f : 0.25f; }

// The initial variance of a valid pixel: the weighted second central moment of l over the valid pixels of the 7x7 window (step 1), weights w_n w_z (1 at the centre).
template <class Taps>
SHM_HD Float denoise_variance_pixel(const Taps& t, const DenoiseConfig& k) {
    DnF4 Bp, Cp;
    if (!t.guides(0, 0, Bp, Cp)) return 0.0f;
    Float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -3; dy <= 3; ++dy)
        for (int dx = -3; dx <= 3; ++dx) {
            DnF4 Bq, Cq;
            if (!t.guides(dx, dy, Bq, Cq)) continue;
            const Float w = (dx == 0 && dy == 0) ? 1.0f : denoise_geometry_weight(Bp, Cp, Bq, Cq, k);
            if (w == 0.0f) continue;
            sw += w;
            s1 += w * Bq.w;
            s2 += w * (Bq.w * Bq.w);
        }
    const Float m1 = s1 / sw, m2 = s2 / sw;
    const Float var = m2 - m1 * m1;
    return var > 0.0f ? var : 0.0f;
}

// One a-trous iteration at a valid pixel, at the taps' spacing: the new plane-A entry (e', var'). A pass-through pixel keeps its zeros.
template <class Taps>
SHM_HD DnF4 denoise_atrous_pixel(const Taps& t, const DenoiseConfig& k) {
    DnF4 Ap, Bp, Cp;
    if (!t.tap(0, 0, Ap, Bp, Cp)) return dn_f4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool use_l = !is_inf(k.sigma_luminance);
    Float inv_l = 0.0f;
    Float wg_inner[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // w_n w_z of the inner ring, which the 5x5 loop takes from here (both loops are unrolled: registers)
    if (use_l) {
        // g3x3(var): the (1, 2, 1) (x) (1, 2, 1) / 16 prefilter of the variance over the 3x3 taps at the iteration's spacing that can be taken, each times its w_n w_z, renormalised
        Float gs = 0.0f, gw = 0.0f;
#pragma unroll
        for (int j = -1; j <= 1; ++j)
#pragma unroll
            for (int i = -1; i <= 1; ++i) {
                DnF4 Aq, Bq, Cq;
                if (!t.tap(i, j, Aq, Bq, Cq)) continue;
                Float g = denoise_g1(j) * denoise_g1(i);
                if (i != 0 || j != 0) {  // (0 across a geometric edge: the other side's variance stays there)
                    wg_inner[(j + 1) * 3 + (i + 1)] = denoise_geometry_weight(Bp, Cp, Bq, Cq, k);
                    g *= wg_inner[(j + 1) * 3 + (i + 1)];
                }
                if (g == 0.0f) continue;
                gs += g * Aq.w;
                gw += g;
            }
        inv_l = k.sigma_luminance * sqrt(gs / gw) + DENOISE_TINY;
    }
    Float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
    for (int j = -2; j <= 2; ++j)
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            DnF4 Aq, Bq, Cq;
            if (!t.tap(i, j, Aq, Bq, Cq)) continue;
            Float w = denoise_h1(j) * denoise_h1(i);
            if (i != 0 || j != 0) {  // the centre tap's weight is h(0, 0) itself
                const bool inner = use_l && i >= -1 && i <= 1 && j >= -1 && j <= 1;
                const Float wg = inner ? wg_inner[(j + 1) * 3 + (i + 1)] : denoise_geometry_weight(Bp, Cp, Bq, Cq, k);
                if (wg == 0.0f) continue;
                w *= wg;
                if (use_l) w *= exp(-(abs(Bp.w - Bq.w) / inv_l));
                if (w == 0.0f) continue;
            }
            sw += w;
            sr += w * Aq.x;
            sg += w * Aq.y;
            sb += w * Aq.z;
            sv += (w * w) * Aq.w;
        }
    return dn_f4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
}

// The result pixel (a ShmFilmPixel's 4 doubles): e a_eff where the filter ran on the pixel, c — bit for bit — where it did not. weight_sum: 1, or 0 where the input's was 0.
SHM_HD void denoise_finish_pixel(const double* film, bool filtered, const DnF4& A, const DnF4& D, double* out) {
    Float c[3];
    denoise_pixel_colour(film, c);
    if (filtered) { c[0] = A.x * D.x; c[1] = A.y * D.y; c[2] = A.z * D.z; }
    out[0] = (double)c[0]; out[1] = (double)c[1]; out[2] = (double)c[2];
    out[3] = film[3] == 0.0 ? 0.0 : 1.0;
}

// The initial variance of a valid pixel from the moments pass's record instead of the spatial estimate (ShmDenoiseParams::variance_source = measured; the caller asks
// for B >= 2). m: a ShmMomentsPixel's twelve doubles (shm/moments.h); D: the pixel's a_eff. With sd_c = sqrt(v_c) the standard deviation of channel c of the pixel's
// mean (0 where v_c is not above 0), the standard deviation of l = mean_c(c_c / a_c) is taken as mean_c(sd_c / a_c) — a path's three channels move together — and the
// variance is its square.
SHM_HD Float denoise_measured_variance(const double* m, const DnF4& D) {
    double v[3], s2[3];
    moments_variances(m, v, s2);
    Float sd[3];
    for (int c = 0; c < 3; ++c) {
        const Float vc = (Float)v[c];
        sd[c] = vc > 0.0f ? sqrt(vc) : 0.0f;
    }
    const Float sd_l = ((sd[0] / D.x + sd[1] / D.y) + sd[2] / D.z) / 3.0f;
    return sd_l * sd_l;
}

}  // namespace shm
