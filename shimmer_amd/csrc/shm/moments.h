// shm/moments.h — the moments pass's arithmetic: per-pixel running mean and variance of the film's batch means, and the tile error an adaptive render stops by
// (include/shimmer_hip.h, shm_moments_* and shm_render_adaptive).
// Single source like every header here: k_moments.hip compiles it for the device, host/host_mirror.cpp for the CPU twin (shm_moments_update_host) and for
// shm_moments_resolve, and the two are held to each other bit for bit (tests/test_gpu_moments.py). Only correctly rounded + - * / in double and conversions between
// double and float: no contraction, no fast-math, no library function.
//
// The pass reads the film and nothing else. A batch's contribution to a pixel is the film after the batch minus the film before it (`prev`), so no render kernel
// knows of it; the recurrence over the batch means x_b with weights dw_b is West's weighted form of Welford's:
//   W' = W + dw;  d = x - mean;  mean' = mean + d (dw / W');  m2' = m2 + (dw d) (x - mean')
// A record is a ShmMomentsPixel's twelve doubles: prev[4] (0..3), mean[3] (4..6), m2[3] (7..9), weight W (10), batches B (11).
#pragma once
#include <vector>
#include "fp.h"

namespace shm {

// ShmAdaptiveParams (include/shimmer_hip.h) as the kernel takes it
struct MomentsConfig {
    int32_t min_batches;  // min_spp / batch_spp
    Float threshold, mean_floor;
};

constexpr int MOMENTS_DOUBLES = 12;

// nullptr, or what is wrong with the parameters (every entry point that takes a ShmAdaptiveParams refuses them with this message)
inline const char* moments_params_error(int32_t min_spp, int32_t batch_spp, Float threshold, Float mean_floor) {
    if (batch_spp < 1) return "adaptive: batch_spp below 1";
    if (min_spp < 2 * batch_spp) return "adaptive: min_spp below 2 * batch_spp (a variance needs two batches)";
    if (min_spp % batch_spp != 0) return "adaptive: min_spp is not a multiple of batch_spp";
    if (!(threshold >= 0.0f)) return "adaptive: threshold is NaN or negative";
    if (!(mean_floor > 0.0f) || is_inf(mean_floor)) return "adaptive: floor is NaN, infinite or not above 0";
    return nullptr;
}

// The tiles of a call as shm_render_wave takes them: inside the bounds, not empty, below 65536, disjoint. tiles: x0, y0, x1, y1 per tile; bitmap: scratch, one bit
// per pixel of the bounds. nullptr, or what is wrong.
inline const char* moments_tiles_error(const int32_t* tiles, uint32_t n_tiles, const int32_t pb[4], std::vector<uint64_t>& bitmap) {
    const uint32_t fw = (uint32_t)(pb[2] - pb[0]);
    const size_t words_per_row = (fw + 63u) / 64u;
    bitmap.assign(words_per_row * (size_t)(pb[3] - pb[1]), 0ull);
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const int32_t tx0 = tiles[4 * t], ty0 = tiles[4 * t + 1], tx1 = tiles[4 * t + 2], ty1 = tiles[4 * t + 3];
        if (tx0 < pb[0] || ty0 < pb[1] || tx1 > pb[2] || ty1 > pb[3] || tx1 <= tx0 || ty1 <= ty0 || tx1 > 65535 || ty1 > 65535 || tx0 < 0 || ty0 < 0)
            return "tile outside pixel bounds";
        const uint32_t x0 = (uint32_t)(tx0 - pb[0]), x1 = (uint32_t)(tx1 - pb[0]);
        for (int y = ty0; y < ty1; ++y) {
            uint64_t* row = bitmap.data() + (size_t)(y - pb[1]) * words_per_row;
            for (uint32_t w0 = x0 / 64u; w0 * 64u < x1; ++w0) {
                const uint32_t lo = (x0 > w0 * 64u ? x0 : w0 * 64u) - w0 * 64u, hi = (x1 < w0 * 64u + 64u ? x1 : w0 * 64u + 64u) - w0 * 64u;  // bits [lo, hi)
                const uint64_t mask = (hi - lo == 64u ? ~0ull : ((1ull << (hi - lo)) - 1ull)) << lo;
                if (row[w0] & mask) return "tiles overlap (each pixel must belong to at most one tile of a call)";
                row[w0] |= mask;
            }
        }
    }
    return nullptr;
}

SHM_HD uint64_t moments_double_bits(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__double_as_longlong(x);
#else
    uint64_t u; memcpy(&u, &x, 8); return u;
#endif
}
SHM_HD bool moments_is_finite(double x) { return (moments_double_bits(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// A record that counts from `film`: nothing seen, prev = the film pixel as it stands
SHM_HD void moments_clear_pixel(const double* film, double* m) {
    for (int c = 0; c < 4; ++c) m[c] = film[c];
    for (int c = 4; c < MOMENTS_DOUBLES; ++c) m[c] = 0.0;
}

// One batch into one record. film: a ShmFilmPixel's 4 doubles (rgb_sum, weight_sum). A batch without positive weight, or whose mean is not finite in some channel, is
// not counted: prev advances and nothing else changes.
SHM_HD void moments_update_pixel(const double* film, double* m) {
    const double dw = film[3] - m[3];
    double x[3];
    bool counted = dw > 0.0;
    for (int c = 0; c < 3; ++c) {
        x[c] = (film[c] - m[c]) / dw;
        counted = counted && moments_is_finite(x[c]);
    }
    for (int c = 0; c < 4; ++c) m[c] = film[c];
    if (!counted) return;
    const double w1 = m[10] + dw;
    const double r = dw / w1;
    for (int c = 0; c < 3; ++c) {
        const double d = x[c] - m[4 + c];
        const double mean1 = m[4 + c] + d * r;
        m[7 + c] = m[7 + c] + (dw * d) * (x[c] - mean1);
        m[4 + c] = mean1;
    }
    m[10] = w1;
    m[11] = m[11] + 1.0;
}

// s2: the per-sample variance m2 / (B - 1); v: the variance of the pixel's mean, s2 / W — both 0 while B < 2. In sensor RGB.
SHM_HD void moments_variances(const double* m, double* v, double* s2) {
    const bool two = m[11] >= 2.0;
    for (int c = 0; c < 3; ++c) {
        s2[c] = two ? m[7 + c] / (m[11] - 1.0) : 0.0;
        v[c] = two ? s2[c] / m[10] : 0.0;
    }
}

// e2: the mean of the three variances of the mean over the square of the mean of the three means, the latter not below `floor`
SHM_HD double moments_e2(const double* m, Float mean_floor) {
    double v[3], s2[3];
    moments_variances(m, v, s2);
    const double mu = ((m[4] + m[5]) + m[6]) / 3.0;
    const double den = mu > (double)mean_floor ? mu : (double)mean_floor;  // (a NaN mean takes the floor)
    return (((v[0] + v[1]) + v[2]) / 3.0) / (den * den);
}

// strictly: threshold 0 converges nothing, +inf everything whose e2 is finite; a NaN e2 never
SHM_HD bool moments_converged(const double* m, double e2, const MomentsConfig& k) {
    return m[11] >= (double)k.min_batches && e2 < (double)k.threshold * (double)k.threshold;
}

// e2 as the tile error carries it: a float, NaN as +inf — and as a key whose unsigned order is the floats' total order (-0 below +0), so that a maximum over
// a tile's pixels is the same bits in whatever order it is taken
SHM_HD Float moments_e2_float(double e2) {
    const Float e = (Float)e2;
    return is_nan(e) ? bits_to_float(0x7f800000u) : e;
}
SHM_HD uint32_t moments_key(Float e) {
    const uint32_t b = float_to_bits(e);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
SHM_HD Float moments_key_value(uint32_t key) { return bits_to_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

// The 8 floats shm_moments_resolve gives for a record: v[3], s2[3], B, e2
SHM_HD void moments_resolve_pixel(const double* m, Float mean_floor, Float* out8) {
    double v[3], s2[3];
    moments_variances(m, v, s2);
    for (int c = 0; c < 3; ++c) {
        out8[c] = (Float)v[c];
        out8[3 + c] = (Float)s2[c];
    }
    out8[6] = (Float)m[11];
    out8[7] = (Float)moments_e2(m, mean_floor);
}

}  // namespace shm
