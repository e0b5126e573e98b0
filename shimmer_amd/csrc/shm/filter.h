// shm/filter.h — the pixel reconstruction filters: box (the reference's one, filter.rs:61-105) and PBRT-v4's gaussian, Mitchell, windowed sinc and triangle
// (pbrt-v4 filters.h / filters.cpp: BoxFilter, GaussianFilter, MitchellFilter, LanczosSincFilter, TriangleFilter, FilterSampler).
//
// A sample is never splatted into neighbouring pixels: the filter is importance-sampled for the film point's offset from the pixel centre and the sample is added to its
// own pixel with weight f / pdf (GetCameraSample). Box and triangle are sampled analytically (weight 1). The other three go through PBRT-v4's FilterSampler: the filter
// tabulated at the centres of int(32 rx) x int(32 ry) cells over [-r, r]^2, a piecewise-constant distribution over the table's ABSOLUTE values, weight = table[cell] / pdf(cell).
// That ratio is +-K with one constant K per table — the integral of |f| —, so the weight is carried as copysign(K, table[cell]) without the per-draw division.
// Every filter here is separable, f(x, y) = g_x(x) g_y(y): the 2-D distribution's marginal over rows is proportional to |g_y| and every row's conditional to |g_x|, so two
// 1-D tables give the same point for the same u as the 2-D table ("Pixel filters": the one stated deviation from PBRT-v4, in layout, not in distribution).
//
// The tables are built on the HOST (filter_build_table: double arithmetic, rounded once), by flatten_scene for the library and the oracle alike; the device only searches them.
#pragma once
#include <math.h>

#include "sampling.h"
#include "scene.h"
#include "spectrum.h"

namespace shm {

// What a kernel is compiled for (k_generate's FC; FILTER_CLASS_ANY: decided at run time from SceneView::filter_kind — the oracle, the probe)
enum : int { FILTER_CLASS_ANY = -1, FILTER_CLASS_BOX = 0, FILTER_CLASS_TRIANGLE = 1, FILTER_CLASS_TABULATED = 2 };
SHM_HD int filter_class_of(uint32_t kind) {
    return kind == SHM_FILTER_BOX ? FILTER_CLASS_BOX : (kind == SHM_FILTER_TRIANGLE ? FILTER_CLASS_TRIANGLE : FILTER_CLASS_TABULATED);
}
// Can two samples of the scene carry different weights? (Mitchell and sinc have negative lobes; gaussian's weight is the one constant K, box's and triangle's 1.)
SHM_HD bool filter_weight_is_signed(uint32_t kind) { return kind == SHM_FILTER_MITCHELL || kind == SHM_FILTER_SINC; }

// A tabulated filter's table, as floats: {K, nx, ny (as integers' bits), 0}, then per axis cdf[n + 1], cdf_low[n + 1], width[n].
//   cdf + cdf_low is the CDF over the cells' absolute values to twice float precision: a cell in the filter's tail holds a few 1e-5 of the probability, and a CDF near 1
//   rounded to a float (spacing 6e-8) puts the inverse off by a few 1e-5 of the radius there — measured against the float64 inverse: Mitchell 2.4e-5 r, a gaussian of radius
//   2.5 5.1e-5 r; with the low word 1.4e-7 r;
//   width[i] = copysign(cdf[i + 1] - cdf[i], g[i]): the cell's probability, with the sign of the filter in the cell (a cell whose entry is 0 has width 0 and is never drawn).
// At most FILTER_MAX_CELLS cells per axis (a radius of 8 pixels): the generate kernels stage the table in LDS.
constexpr int FILTER_TABLE_HEAD = 4, FILTER_MAX_CELLS = 256;
SHM_HD constexpr int filter_table_floats(int nx, int ny) { return FILTER_TABLE_HEAD + 3 * nx + 2 + 3 * ny + 2; }
constexpr int FILTER_TABLE_MAX_FLOATS = filter_table_floats(FILTER_MAX_CELLS, FILTER_MAX_CELLS);
SHM_HD int filter_table_cells(Float radius) {  // FilterSampler: int(32 * radius) (a radius no table is built for — huge, not a number — gives a count above FILTER_MAX_CELLS)
    const Float cells = 32.0f * radius;
    return cells < 1.0e6f ? (int)cells : 1000000;
}

// ---- host: evaluation and table construction ---------------------------------------------------------------------------------
// One axis of the filter at offset x (f(x, y) = g(x; rx) g(y; ry)); a, b: sigma | B, C | tau.
inline double filter_eval_1d(uint32_t kind, double x, double r, double a, double b) {
    const double pi = 3.14159265358979323846;
    const double ax = ::fabs(x);
    switch (kind) {
        case SHM_FILTER_BOX: return ax <= r ? 1.0 : 0.0;
        case SHM_FILTER_GAUSSIAN: {
            auto gauss = [&](double v) { return ::exp(-v * v / (2.0 * a * a)) / ::sqrt(2.0 * pi * a * a); };
            const double g = gauss(x) - gauss(r);
            return g > 0.0 ? g : 0.0;
        }
        case SHM_FILTER_MITCHELL: {
            const double t = ::fabs(2.0 * x / r);
            if (t <= 1.0) return ((12.0 - 9.0 * a - 6.0 * b) * t * t * t + (-18.0 + 12.0 * a + 6.0 * b) * t * t + (6.0 - 2.0 * a)) * (1.0 / 6.0);
            if (t <= 2.0) return ((-a - 6.0 * b) * t * t * t + (6.0 * a + 30.0 * b) * t * t + (-12.0 * a - 48.0 * b) * t + (8.0 * a + 24.0 * b)) * (1.0 / 6.0);
            return 0.0;
        }
        case SHM_FILTER_SINC: {
            if (ax > r) return 0.0;
            auto sinc = [&](double v) { return v == 0.0 ? 1.0 : ::sin(pi * v) / (pi * v); };
            return sinc(x) * sinc(x / a);
        }
        case SHM_FILTER_TRIANGLE: return r - ax > 0.0 ? r - ax : 0.0;
        default: return 0.0;
    }
}
// Fills `out` (FILTER_TABLE_MAX_FLOATS floats at most) for a tabulated kind; returns the number of floats, 0 when a dimension is 0 or above FILTER_MAX_CELLS.
inline int filter_build_table(uint32_t kind, Float rx, Float ry, Float a, Float b, Float* out) {
    const int n[2] = {filter_table_cells(rx), filter_table_cells(ry)};
    if (n[0] < 1 || n[1] < 1 || n[0] > FILTER_MAX_CELLS || n[1] > FILTER_MAX_CELLS) return 0;
    const Float radius[2] = {rx, ry};
    double integral[2];
    int at = FILTER_TABLE_HEAD;
    for (int axis = 0; axis < 2; ++axis) {
        const int m = n[axis];
        const double r = (double)radius[axis];
        Float* cdf = out + at;
        Float* cdf_low = cdf + m + 1;
        Float* width = cdf_low + m + 1;
        // (float entries, as FilterSampler's table holds: the distribution is built over the values the sign is read from; width[] holds them until the sums are through)
        double sum = 0.0;
        for (int i = 0; i < m; ++i) {
            width[i] = (Float)filter_eval_1d(kind, -r + 2.0 * r * ((double)i + 0.5) / (double)m, r, (double)a, (double)b);
            sum += ::fabs((double)width[i]);
        }
        double run = 0.0;
        for (int i = 0; i <= m; ++i) {
            const double c = i == m ? 1.0 : (sum > 0.0 ? run / sum : (double)i / (double)m);
            cdf[i] = (Float)c;
            cdf_low[i] = (Float)(c - (double)cdf[i]);
            if (i < m) {
                const double g = (double)width[i];
                run += ::fabs(g);
                width[i] = (Float)(sum > 0.0 ? g / sum : 1.0 / (double)m);
            }
        }
        integral[axis] = sum * 2.0 * r / (double)m;
        at += 3 * m + 2;
    }
    out[0] = (Float)(integral[0] * integral[1]);  // K
    out[1] = bits_to_float((uint32_t)n[0]);
    out[2] = bits_to_float((uint32_t)n[1]);
    out[3] = 0.0f;
    return at;
}

// ---- host and device: sampling -----------------------------------------------------------------------------------------------
// pbrt-v4 SampleTent (sampling.h): the tent of radius r by the inverse of its CDF
SHM_HD Float sample_tent(Float u, Float r) {
    const Float halves[2] = {0.5f, 0.5f};
    Float up;
    if (sample_discrete(halves, 2, u, nullptr, &up) == 0) return -r + r * sample_linear(up, 0.0f, 1.0f);
    return r * sample_linear(up, 1.0f, 0.0f);
}
// PiecewiseConstant1D::Sample over [-r, r] on one axis of the table: the point, and the filter's sign in its cell
SHM_HD Float filter_sample_axis(const Float* cdf, int n, Float r, Float u, uint32_t& sign) {
    const int cell = find_interval(n + 1, [&](int i) { return cdf[i] <= u; });
    const Float w = cdf[2 * n + 2 + cell];
    Float du = (u - cdf[cell]) - cdf[n + 1 + cell];
    if (w != 0.0f) du /= abs(w);
    sign = float_to_bits(w) & 0x80000000u;
    return lerp(((Float)cell + du) / (Float)n, -r, r);
}
// FilterSampler::Sample on the two 1-D tables (u.y picks the row, u.x the column); weight = copysign(K, g_x[ix] g_y[iy])
SHM_HD void filter_sample_tabulated(const Float* table, Float rx, Float ry, V2 u, V2& p, Float& weight) {
    const int nx = (int)float_to_bits(table[1]), ny = (int)float_to_bits(table[2]);
    uint32_t sx, sy;
    p.y = filter_sample_axis(table + FILTER_TABLE_HEAD + 3 * nx + 2, ny, ry, u.y, sy);
    p.x = filter_sample_axis(table + FILTER_TABLE_HEAD, nx, rx, u.x, sx);
    weight = bits_to_float(float_to_bits(table[0]) | (sx ^ sy));
}
// Filter::Sample(u) -> {p, weight} for a filter of class FC (FILTER_CLASS_ANY: by `kind`). `table`: the tabulated kinds' table (SceneView::dist_data, or a kernel's copy in LDS).
template <int FC = FILTER_CLASS_ANY>
SHM_HD void filter_sample(uint32_t kind, Float rx, Float ry, const Float* table, V2 u, V2& p, Float& weight) {
    const int fc = FC == FILTER_CLASS_ANY ? filter_class_of(kind) : FC;
    if (fc == FILTER_CLASS_BOX) {  // BoxFilter::sample, filter.rs:99-105
        p = v2(lerp(u.x, -rx, rx), lerp(u.y, -ry, ry));
        weight = 1.0f;
    } else if (fc == FILTER_CLASS_TRIANGLE) {
        p = v2(sample_tent(u.x, rx), sample_tent(u.y, ry));
        weight = 1.0f;
    } else {
        filter_sample_tabulated(table, rx, ry, u, p, weight);
    }
}
// ... of the scene's filter (a tabulated filter's table opens the scene's distribution pool: flatten_scene)
SHM_HD void filter_sample(const SceneView& sv, V2 u, V2& p, Float& weight) {
    filter_sample(sv.filter_kind, sv.filter_radius[0], sv.filter_radius[1], sv.dist_data, u, p, weight);
}

}  // namespace shm
