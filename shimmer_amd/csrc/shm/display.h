// shm/display.h — the display pass's arithmetic: a float film into an 8-bit picture — linear output RGB, a log-luminance histogram, the exposure it gives, its
// adaptation over time, a tone curve, the display transfer curve, ordered dither and quantisation (include/shimmer_hip.h, shm_display_*).
// Single source like every header here: k_display.hip compiles it for the device, host/host_mirror.cpp for the CPU twin (shm_display_host), and the two are held to
// each other bit for bit (tests/test_gpu_display.py). All arithmetic is float, in correctly rounded operations and fp.h's own log2 / log / exp / floor / min / max: no
// contraction, no fast-math, no library function. The film's doubles are narrowed exactly as shm_film_get_image narrows them.
//
// Per pixel, in this order:
//   linear     rgb = (float)rgb_sum / (float)weight_sum where weight_sum != 0, times the row-major 3x3 output_rgb_from_sensor_rgb (display_linear_rgb)
//   luminance  Y = 0.2126 R + 0.7152 G + 0.0722 B, left to right
//   bin        256 bins of log2(Y) over [log2_min, log2_max): 0 below, 255 at and above, 1 .. 254 between; a pixel counts iff weight_sum != 0 and Y is finite and > 0
//   exposure   from the 256 counts, by one thread: the mean of the bins' centres over the counted mass between two percentiles; target = log2(key) - mean
//   adapt      adapted = prev + (target - prev) (1 - exp(-rate dt)), or the target itself without a valid previous state; scale = exposure 2^adapted
//   sanitise   c = c scale > 0 ? min(c scale, 65504) : 0
//   tone       none, extended Reinhard on luminance, or Narkowicz's ACES fit per channel; then a clamp to [0, 1]
//   transfer   linear or sRGB
//   quantise   floor(v 255 + 0.5), or floor(v 255 + (b(x, y) + 0.5) / 64) with the 8x8 Bayer matrix b; bytes R, G, B, 255
#pragma once
#include "fp.h"

namespace shm {

constexpr uint32_t DISPLAY_SOURCE_FILM = 0u, DISPLAY_SOURCE_DENOISED = 1u, DISPLAY_SOURCE_TEMPORAL = 2u;
constexpr uint32_t DISPLAY_TONEMAP_NONE = 0u, DISPLAY_TONEMAP_REINHARD = 1u, DISPLAY_TONEMAP_ACES = 2u;
constexpr uint32_t DISPLAY_TRANSFER_LINEAR = 0u, DISPLAY_TRANSFER_SRGB = 1u;
constexpr int DISPLAY_BINS = 256;
constexpr Float DISPLAY_MAX_VALUE = 65504.0f;  // the reference's f16 cap (film.rs:676-690)
constexpr Float DISPLAY_LN2 = 0.69314718055994530942f;

// ShmDisplayParams (include/shimmer_hip.h) as the kernels take it
struct DisplayConfig {
    uint32_t tonemap, transfer, dither;
    Float exposure, key, white, log2_min, log2_max, percentile_low, percentile_high, adaptation_rate, dt;
    Float m[9];  // output_rgb_from_sensor_rgb, row-major
};
// The adaptation's state: what one frame leaves for the next
struct DisplayAdaptation {
    Float log2_exposure;
    uint32_t valid;
};

// nullptr, or what is wrong with the parameters (every entry point that takes a ShmDisplayParams refuses them with this message)
inline const char* display_params_error(uint32_t source, const DisplayConfig& k) {
    if (source > DISPLAY_SOURCE_TEMPORAL) return "display: unknown source";
    if (k.tonemap > DISPLAY_TONEMAP_ACES) return "display: unknown tonemap";
    if (k.transfer > DISPLAY_TRANSFER_SRGB) return "display: unknown transfer";
    if (!is_finite(k.log2_min) || !is_finite(k.log2_max) || !(k.log2_min < k.log2_max)) return "display: log2_min is not below log2_max (or one is not finite)";
    if (!(k.percentile_low >= 0.0f && k.percentile_low < k.percentile_high && k.percentile_high <= 1.0f)) return "display: the percentiles are not 0 <= low < high <= 1";
    if (!is_finite(k.exposure) || !(k.exposure > 0.0f)) return "display: exposure is not finite or not above 0";
    if (!is_finite(k.key) || !(k.key > 0.0f)) return "display: key is not finite or not above 0";
    if (!is_finite(k.white) || !(k.white > 0.0f)) return "display: white is not finite or not above 0";
    if (!is_finite(k.dt)) return "display: dt is not finite";
    if (!is_finite(k.adaptation_rate)) return "display: adaptation_rate is not finite";
    for (int i = 0; i < 9; ++i)
        if (!is_finite(k.m[i])) return "display: output_rgb_from_sensor_rgb has an entry that is not finite";
    return nullptr;
}

// RgbFilm::get_pixel_rgb and the output matrix, as shm_film_get_image with write_fp16 = 0 has them (host/host_mirror.cpp): film: a ShmFilmPixel's 4 doubles
SHM_HD void display_linear_rgb(const double* film, const Float* m, Float* out) {
    Float rgb[3] = {(Float)film[0], (Float)film[1], (Float)film[2]};
    if (film[3] != 0.0) {
        const Float w = (Float)film[3];
        rgb[0] /= w; rgb[1] /= w; rgb[2] /= w;
    }
    for (int c = 0; c < 3; ++c) rgb[c] += 0.0f;  // (the splat term, always zero here; it turns -0 into +0 as it does there)
    for (int r = 0; r < 3; ++r) {
        Float acc = 0.0f;
        for (int c = 0; c < 3; ++c) acc += m[3 * r + c] * rgb[c];
        out[r] = acc;
    }
}

SHM_HD Float display_luminance(const Float* c) { return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2]; }

// bins per unit of log2 luminance, and a bin's centre (bins 0 and 255: the range's two ends)
SHM_HD Float display_bins_per_stop(Float log2_min, Float log2_max) { return 254.0f / (log2_max - log2_min); }
SHM_HD Float display_bin_centre(int b, Float log2_min, Float log2_max) {
    if (b <= 0) return log2_min;
    if (b >= DISPLAY_BINS - 1) return log2_max;
    return log2_min + ((Float)b - 0.5f) * ((log2_max - log2_min) / 254.0f);
}

// The bin a pixel is counted in, or -1 for one that is not counted. weight: the film's weight_sum; Y: display_luminance of its linear output RGB.
SHM_HD int display_bin(double weight, Float Y, Float log2_min, Float log2_max) {
    if (weight == 0.0 || !is_finite(Y) || !(Y > 0.0f)) return -1;
    const Float l = log2(Y);
    if (l < log2_min) return 0;
    if (l >= log2_max) return DISPLAY_BINS - 1;
    const int b = 1 + (int)floor((l - log2_min) * display_bins_per_stop(log2_min, log2_max));
    return b < 1 ? 1 : (b > DISPLAY_BINS - 2 ? DISPLAY_BINS - 2 : b);
}

// The target log2 exposure from the 256 counts, in bin order (one thread): the mean of the bins' centres over the counted mass between percentile_low N and
// percentile_high N, a bin that straddles either end counted by the part inside. counted_out: N.
SHM_HD Float display_exposure_target(const uint32_t* counts, const DisplayConfig& k, uint32_t& counted_out) {
    uint32_t n = 0;
#pragma unroll 16
    for (int b = 0; b < DISPLAY_BINS; ++b) n += counts[b];
    counted_out = n;
    if (n == 0) return 0.0f;
    const Float lo = k.percentile_low * (Float)n, hi = k.percentile_high * (Float)n;
    Float before = 0.0f, mass = 0.0f, sum = 0.0f;
    Float at_lo = k.log2_min;  // the centre of the bin that holds the low percentile: the mean where rounding leaves no mass between the two
    bool have_lo = false;
    // (no branch on an empty bin, so that the one device thread that runs this has its loads of `counts` batched: an empty bin has after == before, and
    // min(after, hi) <= before <= max(before, lo) adds nothing)
#pragma unroll 8
    for (int b = 0; b < DISPLAY_BINS; ++b) {
        const Float after = before + (Float)counts[b];
        const Float centre = display_bin_centre(b, k.log2_min, k.log2_max);
        if (!have_lo && counts[b] != 0 && after >= lo) { at_lo = centre; have_lo = true; }
        const Float a = before > lo ? before : lo, e = after < hi ? after : hi;  // (all four finite)
        const Float part = e > a ? e - a : 0.0f;
        mass += part;
        sum += part * centre;
        before = after;
    }
    const Float mean = mass > 0.0f ? sum / mass : at_lo;
    return log2(k.key) - mean;
}

// One frame of adaptation: the exposure moves towards `target` by 1 - exp(-rate dt) of the way; a state that is not valid, dt <= 0 or rate <= 0 jump. Returns the
// scale and advances `state`.
SHM_HD Float display_adapt(Float target, const DisplayConfig& k, DisplayAdaptation& state) {
    Float adapted = target;
    if (state.valid && k.dt > 0.0f && k.adaptation_rate > 0.0f) {
        const Float prev = state.log2_exposure;
        adapted = prev + (target - prev) * (1.0f - exp(-k.adaptation_rate * k.dt));
    }
    state.log2_exposure = adapted;
    state.valid = 1u;
    return k.exposure * exp(adapted * DISPLAY_LN2);
}

SHM_HD Float display_srgb(Float v) { return v <= 0.0031308f ? 12.92f * v : 1.055f * exp(log(v) * (1.0f / 2.4f)) - 0.055f; }
SHM_HD Float display_aces(Float x) { return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f); }

// The recursive 8x8 Bayer matrix: each of 0 .. 63 once. The bits of x ^ y and of y, interleaved from the least significant pair to the most significant place.
SHM_HD uint32_t display_bayer8(uint32_t x, uint32_t y) {
    const uint32_t a = (x ^ y) & 7u, b = y & 7u;
    return ((a & 1u) << 5) | ((b & 1u) << 4) | ((a & 2u) << 2) | ((b & 2u) << 1) | ((a & 4u) >> 1) | ((b & 4u) >> 2);
}

// Linear output RGB to the pixel's four bytes R, G, B, 255 as one little-endian word. x, y: the pixel's film coordinates (the dither's).
SHM_HD uint32_t display_map_pixel(const Float* linear, Float scale, uint32_t x, uint32_t y, const DisplayConfig& k) {
    Float c[3];
    for (int i = 0; i < 3; ++i) {
        const Float s = linear[i] * scale;
        c[i] = s > 0.0f ? min(s, DISPLAY_MAX_VALUE) : 0.0f;  // (NaN and negative: 0; +inf: the cap)
    }
    if (k.tonemap == DISPLAY_TONEMAP_REINHARD) {
        const Float Y = display_luminance(c);
        if (Y > 0.0f) {
            const Float Yd = (Y * (1.0f + Y / (k.white * k.white))) / (1.0f + Y);
            const Float r = Yd / Y;
            for (int i = 0; i < 3; ++i) c[i] = c[i] * r;
        }
    } else if (k.tonemap == DISPLAY_TONEMAP_ACES) {
        for (int i = 0; i < 3; ++i) c[i] = display_aces(c[i]);
    }
    const Float bias = k.dither ? ((Float)display_bayer8(x, y) + 0.5f) / 64.0f : 0.5f;
    uint32_t word = 0xff000000u;
    for (int i = 0; i < 3; ++i) {
        Float v = min(max(c[i], 0.0f), 1.0f);  // (fp.h's max drops a NaN: 0)
        if (k.transfer == DISPLAY_TRANSFER_SRGB) v = display_srgb(v);
        int code = (int)floor(v * 255.0f + bias);
        code = code < 0 ? 0 : (code > 255 ? 255 : code);
        word |= (uint32_t)code << (8 * i);
    }
    return word;
}

}  // namespace shm
