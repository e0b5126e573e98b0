// k_display.hip — the display pass's three kernels and its device entry points (include/shimmer_hip.h, shm_display_*). The arithmetic is
// shm/display.h, which host/host_mirror.cpp compiles a second time for the CPU twin; the kernels here only say which pixels a lane owns and how the counts travel.
//   k_display_histogram   workgroups of 256 lanes, each over a contiguous run of pixels (a multiple of 256; lane l takes the run's pixels l, l + 256, ...: coalesced
//                         32-byte loads, four pixels' in flight). Every wave bins into its own 256-word LDS histogram with integer LDS adds; after a barrier lane b
//                         sums bin b over the four and writes it to the workgroup's 1 KB slab with a plain vector store. No global atomics, no float atomics: the
//                         counts are integers, so no order matters.
//   k_display_exposure    one workgroup of 256 lanes. Lane b sums bin b over the slabs (32 loads in flight) and writes the count; after a barrier lane 0 runs
//                         display_exposure_target and display_adapt over the 256 counts in LDS and writes the state. No host round trip between the passes.
//                         The pass's longest kernel, by latency: profiles/display.md.
//   k_display_map         one pixel per lane: 32 bytes in, one coalesced uint32_t out. The scale is a wave-uniform load from the state.
// With auto_exposure = 0 only k_display_map runs, and its scale is the exposure.
// The pass reads one of the film, the denoiser's result and the temporal pass's, and writes only its own buffers. This unit draws no sample and shades nothing: it sets
// none of the shared headers' switches, and its name matches none of the Makefile's *_zs / *_dl patterns.
#include "wavefront.h"
#include "shm/display.h"

namespace {

constexpr int DP_LANES = 256, DP_WAVES = DP_LANES / 64;
constexpr uint32_t DP_MAX_SLABS = 256;  // a workgroup per CU: 256 KB of slabs for k_display_exposure's one workgroup to sum (profiles/display.md: with 512 slabs summed
                                        // eight loads at a time that kernel took 47 us of the pass's 71)
constexpr uint32_t DP_SUM_BATCH = 32, DP_PIXEL_BATCH = 4;
static_assert(DISPLAY_BINS == DP_LANES, "lane b owns bin b");
static_assert(sizeof(ShmFilmPixel) == 4 * sizeof(double), "the pixel functions of shm/display.h index the film as doubles");
static_assert(sizeof(ShmDisplayParams) == 96 && sizeof(ShmDisplayState) == 32, "include/shimmer_hip.h: the display structs' layout");
static_assert(SHM_DISPLAY_SOURCE_TEMPORAL == DISPLAY_SOURCE_TEMPORAL && SHM_TONEMAP_ACES == DISPLAY_TONEMAP_ACES && SHM_TRANSFER_SRGB == DISPLAY_TRANSFER_SRGB,
              "shm/display.h restates the header's constants");

// a film pixel as two 16-byte loads
__device__ inline void load_pixel(const ShmFilmPixel* film, size_t q, double* f) {
    const double2* p = reinterpret_cast<const double2*>(film + q);
    const double2 a = p[0], b = p[1];
    f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y;
}

__global__ void __launch_bounds__(DP_LANES) k_display_histogram(const ShmFilmPixel* film, uint32_t n, uint32_t run, DisplayConfig k, uint32_t* slabs) {
    __shared__ uint32_t hist[DP_WAVES][DISPLAY_BINS];
    const uint32_t lane = threadIdx.x;
    for (int w = 0; w < DP_WAVES; ++w) hist[w][lane] = 0u;
    __syncthreads();
    uint32_t* mine = hist[lane / 64u];
    const uint32_t begin = blockIdx.x * run;  // (begin < n and run <= n + 256: no sum below overflows under 2^31 pixels, and ensure_display refuses more)
    const uint32_t end = begin + run < n ? begin + run : n;
    for (uint32_t q0 = begin + lane; q0 < end; q0 += DP_PIXEL_BATCH * DP_LANES) {
        double f[DP_PIXEL_BATCH][4];  // four pixels' loads in flight before the first is binned
#pragma unroll
        for (uint32_t j = 0; j < DP_PIXEL_BATCH; ++j) {
            const uint32_t q = q0 + j * DP_LANES;
            if (q < end) load_pixel(film, q, f[j]);
            else f[j][0] = f[j][1] = f[j][2] = f[j][3] = 0.0;  // (no weight: not counted)
        }
#pragma unroll
        for (uint32_t j = 0; j < DP_PIXEL_BATCH; ++j) {
            Float c[3];
            display_linear_rgb(f[j], k.m, c);
            const int b = display_bin(f[j][3], display_luminance(c), k.log2_min, k.log2_max);
            if (b >= 0) atomicAdd(&mine[b], 1u);  // (b in [0, 255]: display_bin clamps)
        }
    }
    __syncthreads();
    uint32_t total = 0;
    for (int w = 0; w < DP_WAVES; ++w) total += hist[w][lane];
    slabs[(size_t)blockIdx.x * DISPLAY_BINS + lane] = total;
}

__global__ void __launch_bounds__(DP_LANES) k_display_exposure(const uint32_t* slabs, uint32_t n_slabs, DisplayConfig k, uint32_t* state) {
    __shared__ uint32_t counts[DISPLAY_BINS];
    const uint32_t lane = threadIdx.x;
    // one workgroup reads every slab, so what bounds it is a load's latency times the loads a lane issues one behind the other: 32 in flight per lane
    uint32_t total = 0, s = 0;
    for (; s + DP_SUM_BATCH <= n_slabs; s += DP_SUM_BATCH) {
        uint32_t v[DP_SUM_BATCH];
#pragma unroll
        for (uint32_t j = 0; j < DP_SUM_BATCH; ++j) v[j] = slabs[(size_t)(s + j) * DISPLAY_BINS + lane];
#pragma unroll
        for (uint32_t j = 0; j < DP_SUM_BATCH; ++j) total += v[j];
    }
    for (; s < n_slabs; ++s) total += slabs[(size_t)s * DISPLAY_BINS + lane];
    counts[lane] = total;
    state[lane] = total;
    __syncthreads();
    if (lane != 0) return;
    ShmDisplayState* st = reinterpret_cast<ShmDisplayState*>(state + DISPLAY_BINS);
    DisplayAdaptation a{st->log2_exposure, st->valid};
    uint32_t counted = 0;
    const Float target = display_exposure_target(counts, k, counted);
    const Float scale = display_adapt(target, k, a);
    st->log2_target = target;
    st->log2_exposure = a.log2_exposure;
    st->scale = scale;
    st->counted = counted;
    st->valid = a.valid;
}

__global__ void __launch_bounds__(DP_LANES) k_display_map(const ShmFilmPixel* film, uint32_t n, uint32_t width, const uint32_t* state /* null: scale = exposure */,
                                                          DisplayConfig k, uint32_t* out) {
    const uint32_t q = blockIdx.x * DP_LANES + threadIdx.x;
    if (q >= n) return;
    const Float scale = state ? reinterpret_cast<const ShmDisplayState*>(state + DISPLAY_BINS)->scale : k.exposure;
    double f[4];
    Float c[3];
    load_pixel(film, q, f);
    display_linear_rgb(f, k.m, c);
    out[q] = display_map_pixel(c, scale, q % width, q / width, k);
}

DisplayConfig display_config(const ShmDisplayParams& p) {
    DisplayConfig k{p.tonemap, p.transfer, p.dither ? 1u : 0u, p.exposure, p.key, p.white, p.log2_min, p.log2_max, p.percentile_low, p.percentile_high, p.adaptation_rate, p.dt, {}};
    for (int i = 0; i < 9; ++i) k.m[i] = p.output_rgb_from_sensor_rgb[i];
    return k;
}

// the histogram's grid: one workgroup per 256 pixels up to DP_MAX_SLABS, then longer runs
void histogram_grid(size_t n, uint32_t& n_slabs, uint32_t& run) {
    const size_t groups = std::max<size_t>((n + DP_LANES - 1) / DP_LANES, 1);
    n_slabs = (uint32_t)std::min<size_t>(groups, DP_MAX_SLABS);
    run = (uint32_t)((groups + n_slabs - 1) / n_slabs) * DP_LANES;
    n_slabs = (uint32_t)((groups * DP_LANES + run - 1) / run);  // (no empty workgroup behind the last pixel)
}

constexpr size_t STATE_BYTES = DISPLAY_BINS * sizeof(uint32_t) + sizeof(ShmDisplayState);

// the image, the slabs and the counts + state: one allocation, the scene's to free; counts and state zeroed
int ensure_display(ShmScene* s) {
    if (s->d_display) return SHM_OK;
    const size_t n = s->n_film_pixels;
    if (n >= ((size_t)1 << 31)) { shm_err() = "display: more pixels than the pass indexes with 32 bits"; return SHM_ERR_UNSUPPORTED; }
    const size_t image_words = (std::max<size_t>(n, 1) + 63) & ~(size_t)63;  // (the slabs behind it start on 256 bytes)
    void* d = nullptr;
    int rc;
    if ((rc = wf_scene_alloc(s, (image_words + (size_t)DP_MAX_SLABS * DISPLAY_BINS) * sizeof(uint32_t) + STATE_BYTES, &d)) != SHM_OK) return rc;
    uint32_t* base = reinterpret_cast<uint32_t*>(d);
    if (hipMemsetAsync(base + image_words + (size_t)DP_MAX_SLABS * DISPLAY_BINS, 0, STATE_BYTES, s->stream) != hipSuccess) {
        wf_scene_free(s, d);
        shm_err() = "hipMemset of the display state";
        return SHM_ERR_DEVICE;
    }
    s->d_display = base;
    s->d_display_slabs = base + image_words;
    s->d_display_state = s->d_display_slabs + (size_t)DP_MAX_SLABS * DISPLAY_BINS;
    return SHM_OK;
}

}  // namespace

extern "C" {

int shm_display_clear(ShmScene* s) {
    if (!s) { shm_err() = "display: no scene"; return SHM_ERR_INVALID_ARGUMENT; }
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_display(s)) != SHM_OK) return rc;
    HIP_TRY(hipMemsetAsync(s->d_display_state, 0, STATE_BYTES, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SHM_OK;
}

int shm_display_device(ShmScene* s, const ShmDisplayParams* params, ShmDisplayState* state_out, double* ms_out) {
    if (!s || !params) { shm_err() = "display: no scene or no parameters"; return SHM_ERR_INVALID_ARGUMENT; }
    const DisplayConfig k = display_config(*params);
    if (const char* why = display_params_error(params->source, k)) { shm_err() = why; return SHM_ERR_INVALID_ARGUMENT; }
    const ShmFilmPixel* src = s->d_film;
    if (params->source == SHM_DISPLAY_SOURCE_DENOISED) {
        if (!s->d_denoised || !s->denoised) { shm_err() = "display: source is the denoiser's result, and the scene holds none (no shm_denoise_device yet)"; return SHM_ERR_INVALID_ARGUMENT; }
        src = s->d_denoised;
    } else if (params->source == SHM_DISPLAY_SOURCE_TEMPORAL) {
        if (!s->d_temporal_out || !s->temporal_filled) { shm_err() = "display: source is the temporal result, and the scene holds none (no shm_temporal_accumulate_device since the scene was created or the history cleared)"; return SHM_ERR_INVALID_ARGUMENT; }
        src = s->d_temporal_out;
    }
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_display(s)) != SHM_OK) return rc;
    const uint32_t n = (uint32_t)s->n_film_pixels;
    const int32_t* pb = s->flat.film.pixel_bounds;
    const uint32_t width = (uint32_t)std::max(pb[2] - pb[0], 1);
    EventPool ev{s};
    hipEvent_t e_begin = ev.get(), e_end = ev.get();
    if (ev.failed) { shm_err() = "hipEventCreate failed"; return SHM_ERR_DEVICE; }
    const bool metered = params->auto_exposure != 0;
    HIP_TRY(hipEventRecord(e_begin, s->stream));
    if (metered) {
        uint32_t n_slabs, run;
        histogram_grid(n, n_slabs, run);
        hipLaunchKernelGGL(k_display_histogram, dim3(n_slabs), dim3(DP_LANES), 0, s->stream, src, n, run, k, s->d_display_slabs);
        LAUNCH_TRY("k_display_histogram");
        hipLaunchKernelGGL(k_display_exposure, dim3(1), dim3(DP_LANES), 0, s->stream, s->d_display_slabs, n_slabs, k, s->d_display_state);
        LAUNCH_TRY("k_display_exposure");
    }
    if (n > 0) {
        hipLaunchKernelGGL(k_display_map, dim3((n + DP_LANES - 1) / DP_LANES), dim3(DP_LANES), 0, s->stream, src, n, width, metered ? s->d_display_state : nullptr, k, s->d_display);
        LAUNCH_TRY("k_display_map");
    }
    HIP_TRY(hipEventRecord(e_end, s->stream));
    if (state_out) HIP_TRY(hipMemcpyAsync(state_out, s->d_display_state + DISPLAY_BINS, sizeof(ShmDisplayState), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    s->display_filled = true;
    if (ms_out) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, e_begin, e_end));
        *ms_out = (double)ms;
    }
    return SHM_OK;
}

int shm_display_read(ShmScene* s, uint32_t* out) {
    if (!s || !out) { shm_err() = "display: a null argument"; return SHM_ERR_INVALID_ARGUMENT; }
    if (!s->display_filled) { shm_err() = "display: nothing to read before shm_display_device"; return SHM_ERR_INVALID_ARGUMENT; }
    return wf_read_pixels(s, s->d_display, sizeof(uint32_t), out);
}

int shm_display_read_histogram(ShmScene* s, uint32_t* counts_out) {
    if (!s || !counts_out) { shm_err() = "display: a null argument"; return SHM_ERR_INVALID_ARGUMENT; }
    if (!s->display_filled) { shm_err() = "display: nothing to read before shm_display_device"; return SHM_ERR_INVALID_ARGUMENT; }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(counts_out, s->d_display_state, DISPLAY_BINS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SHM_OK;
}

int shm_display_device_ptr(ShmScene* s, void** ptr_out, uint64_t* bytes_out) {
    if (!s || !ptr_out || !bytes_out) { shm_err() = "display: a null argument"; return SHM_ERR_INVALID_ARGUMENT; }
    if (!s->d_display) { shm_err() = "display: no image buffer before shm_display_device or shm_display_clear"; return SHM_ERR_INVALID_ARGUMENT; }
    *ptr_out = s->d_display;
    *bytes_out = (uint64_t)(s->n_film_pixels * sizeof(uint32_t));
    return SHM_OK;
}

int shm_display(ShmScene* s, const ShmDisplayParams* params, uint32_t* rgba8_out, ShmDisplayState* state_out, double* ms_out) {
    if (!rgba8_out) { shm_err() = "display: no image to write to"; return SHM_ERR_INVALID_ARGUMENT; }
    const int rc = shm_display_device(s, params, state_out, ms_out);
    return rc != SHM_OK ? rc : shm_display_read(s, rgba8_out);
}

}  // extern "C"
