// k_temporal.hip — the temporal pass's two kernels and its device entry points (include/shimmer_hip.h, shm_temporal_* and
// shm_denoise_temporal_device). The arithmetic is shm/temporal.h, which host/host_mirror.cpp compiles a second time for the CPU twin; the kernels here only say which
// pixel a lane owns.
//   k_temporal_accumulate   one 64-lane workgroup — one wave — per 8x8 tile of the film, one pixel per lane (a clipped edge tile leaves lanes idle). A streaming
//                           gather: the lane reads its film pixel (32 bytes) and its G-buffer pixel (128), up to four records of the previous frame where the motion
//                           sends it (three 16-byte loads each: the pad word is not read), and writes its own record (four 16-byte stores) and its result (32 bytes).
//                           No LDS — the taps of a tile lie wherever the camera's motion puts them —, no atomics, no cross-lane dependence: a lane never writes
//                           what another reads, because the records it reads are the OTHER array's.
//   k_temporal_variance     one pixel per lane, behind the denoiser's variance pass when shm_denoise_temporal_device asks: max(0, m2 - m1^2) / length over plane A's
//                           variance at every valid pixel whose record has length >= 4
// The two cameras travel as kernel arguments (two 132-byte structs): the host inverts each camera_from_raster once, in double.
// This unit draws no sample and shades nothing: it sets none of the shared headers' switches, and its name matches none of the Makefile's *_zs / *_dl patterns.
#include "wavefront.h"
#include "shm/temporal.h"

namespace {

constexpr int TP_TILE = 8, TP_WAVE = TP_TILE * TP_TILE;
static_assert(sizeof(ShmFilmPixel) == 4 * sizeof(double) && sizeof(ShmGBufferPixel) == 16 * sizeof(double), "the pixel functions of shm/denoise.h index the sums as doubles");
static_assert(sizeof(ShmTemporalPixel) == 64 && sizeof(TemporalRecord) == 64 && sizeof(ShmTemporalParams) == 32, "include/shimmer_hip.h: the temporal structs' layout");
static_assert(sizeof(DnF4) == sizeof(float4), "a record word is a float4");

__global__ void __launch_bounds__(TP_WAVE) k_temporal_accumulate(const ShmFilmPixel* film, const ShmGBufferPixel* gbuffer, const TemporalRecord* history /* null: none */,
                                                                 TemporalCamera cur, TemporalCamera prev, int width, int height, float white_r, float white_g, float white_b,
                                                                 TemporalConfig k, TemporalRecord* records, ShmFilmPixel* out) {
    const int lane = (int)threadIdx.x;
    const int x = (int)blockIdx.x * TP_TILE + lane % TP_TILE, y = (int)blockIdx.y * TP_TILE + lane / TP_TILE;
    if (x >= width || y >= height) return;
    const size_t q = (size_t)y * (size_t)width + (size_t)x;
    const float white[3] = {white_r, white_g, white_b};
    double f[4], g[16], o[4];
    const double* fp = reinterpret_cast<const double*>(film + q);
    const double* gp = reinterpret_cast<const double*>(gbuffer + q);
    for (int c = 0; c < 4; ++c) f[c] = fp[c];
    for (int c = 0; c < 16; ++c) g[c] = gp[c];
    TemporalRecord rec;
    temporal_pixel(f, g, white, history, cur, prev, x, y, width, height, k, rec, o);
    TemporalRecord* r = records + q;
    r->a = rec.a; r->b = rec.b; r->c = rec.c; r->d = rec.d;
    out[q].rgb_sum[0] = o[0]; out[q].rgb_sum[1] = o[1]; out[q].rgb_sum[2] = o[2]; out[q].weight_sum = o[3];
}

__global__ void __launch_bounds__(256) k_temporal_variance(DnF4* A, const DnF4* C, const TemporalRecord* records, uint32_t n) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n || C[q].w == 0.0f) return;
    TemporalRecord t;
    t.a = records[q].a; t.b = records[q].b;
    if (!(t.b.y >= TEMPORAL_VARIANCE_MIN_LENGTH)) return;  // a short history: the spatial estimate stays
    A[q].w = temporal_variance(t);
}

TemporalConfig temporal_config(const ShmTemporalParams& p) {
    return TemporalConfig{p.alpha_min, p.alpha_min_moments, p.max_history, p.normal_cos_min, p.plane_tolerance, p.albedo_floor, p.demodulate};
}

// the two record arrays and the result: one allocation, the scene's to free; both arrays emptied
int ensure_temporal(ShmScene* s) {
    if (s->d_temporal[0]) return SHM_OK;
    const size_t n = std::max<size_t>(s->n_film_pixels, 1);
    void* d = nullptr;
    int rc;
    if ((rc = wf_scene_alloc(s, n * (2 * sizeof(TemporalRecord) + sizeof(ShmFilmPixel)), &d)) != SHM_OK) return rc;
    if (hipMemsetAsync(d, 0, n * (2 * sizeof(TemporalRecord) + sizeof(ShmFilmPixel)), s->stream) != hipSuccess) { wf_scene_free(s, d); shm_err() = "hipMemset of the temporal history"; return SHM_ERR_DEVICE; }
    s->d_temporal[0] = reinterpret_cast<float4*>(d);
    s->d_temporal[1] = s->d_temporal[0] + 4 * n;
    s->d_temporal_out = reinterpret_cast<ShmFilmPixel*>(s->d_temporal[1] + 4 * n);
    return SHM_OK;
}

}  // namespace

int wf_launch_temporal_variance(hipStream_t stream, float4* A, const float4* C, const float4* temporal_records, uint32_t n) {
    hipLaunchKernelGGL(k_temporal_variance, dim3((n + 255u) / 256u), dim3(256), 0, stream, reinterpret_cast<DnF4*>(A), reinterpret_cast<const DnF4*>(C),
                       reinterpret_cast<const TemporalRecord*>(temporal_records), n);
    LAUNCH_TRY("k_temporal_variance");
    return SHM_OK;
}

extern "C" {

int shm_temporal_default_params(ShmTemporalParams* out) {
    if (!out) return SHM_ERR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    out->alpha_min = 0.2f;
    out->alpha_min_moments = 0.2f;
    out->max_history = 32.0f;
    out->normal_cos_min = 0.9f;
    out->plane_tolerance = 0.02f;
    out->albedo_floor = 0.01f;
    out->demodulate = 0;
    return SHM_OK;
}

int shm_temporal_clear(ShmScene* s) {
    if (!s) { shm_err() = "temporal: no scene"; return SHM_ERR_INVALID_ARGUMENT; }
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_temporal(s)) != SHM_OK) return rc;
    // (zero records: every length is 0; the result goes with them)
    HIP_TRY(hipMemsetAsync(s->d_temporal[0], 0, std::max<size_t>(s->n_film_pixels, 1) * (2 * sizeof(TemporalRecord) + sizeof(ShmFilmPixel)), s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->temporal_has_camera = false;
    s->temporal_filled = false;
    s->temporal_cur = 0;
    return SHM_OK;
}

int shm_temporal_accumulate_device(ShmScene* s, const ShmTemporalParams* params, double* ms_out) {
    if (!s || !params) { shm_err() = "temporal: no scene or no parameters"; return SHM_ERR_INVALID_ARGUMENT; }
    const TemporalConfig k = temporal_config(*params);
    if (const char* why = temporal_params_error(k)) { shm_err() = why; return SHM_ERR_INVALID_ARGUMENT; }
    const ShmCamera& cam = s->flat.camera;
    if (cam.kind == SHM_CAMERA_SPHERICAL) { shm_err() = "temporal: the spherical camera is not reprojected"; return SHM_ERR_UNSUPPORTED; }
    if (!s->d_gbuffer || !s->gbuffer_filled) {
        shm_err() = "temporal: the scene's G-buffer is empty (no shm_gbuffer_render_wave / shm_render_gbuffer since the scene was created or the G-buffer cleared)";
        return SHM_ERR_INVALID_ARGUMENT;
    }
    if (s->gbuffer_space != SHM_GBUFFER_SPACE_RENDER) { shm_err() = "temporal: the last G-buffer wave was not in SHM_GBUFFER_SPACE_RENDER"; return SHM_ERR_INVALID_ARGUMENT; }
    TemporalCamera cur, prev;
    if (!temporal_camera(cam.camera_from_raster, cam.camera_from_render, cam.kind == SHM_CAMERA_PERSPECTIVE, cur)) { shm_err() = "temporal: camera_from_raster is singular"; return SHM_ERR_INVALID_ARGUMENT; }
    prev = cur;
    const bool has_history = s->temporal_has_camera;
    if (has_history) {
        const ShmCamera& pc = s->temporal_camera;
        if (!temporal_camera(pc.camera_from_raster, pc.camera_from_render, pc.kind == SHM_CAMERA_PERSPECTIVE, prev)) { shm_err() = "temporal: the previous camera_from_raster is singular"; return SHM_ERR_INVALID_ARGUMENT; }
    }
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_temporal(s)) != SHM_OK) return rc;
    const int32_t* pb = s->flat.film.pixel_bounds;
    const int width = pb[2] - pb[0], height = pb[3] - pb[1];
    double white[3] = {0.0, 0.0, 0.0};  // shm_gbuffer_white
    const std::vector<float>* tables[3] = {&s->flat.sensor_r, &s->flat.sensor_g, &s->flat.sensor_b};
    for (int c = 0; c < 3; ++c)
        for (float v : *tables[c]) white[c] += (double)v;
    EventPool ev{s};
    hipEvent_t e_begin = ev.get(), e_end = ev.get();
    if (ev.failed) { shm_err() = "hipEventCreate failed"; return SHM_ERR_DEVICE; }
    const int from = s->temporal_cur, to = has_history ? from ^ 1 : from;
    const TemporalRecord* history = has_history ? reinterpret_cast<const TemporalRecord*>(s->d_temporal[from]) : nullptr;
    HIP_TRY(hipEventRecord(e_begin, s->stream));
    if (width > 0 && height > 0) {
        const dim3 grid((unsigned)((width + TP_TILE - 1) / TP_TILE), (unsigned)((height + TP_TILE - 1) / TP_TILE));
        hipLaunchKernelGGL(k_temporal_accumulate, grid, dim3(TP_WAVE), 0, s->stream, s->d_film, s->d_gbuffer, history, cur, prev, width, height, (float)white[0], (float)white[1],
                           (float)white[2], k, reinterpret_cast<TemporalRecord*>(s->d_temporal[to]), s->d_temporal_out);
        LAUNCH_TRY("k_temporal_accumulate");
    }
    HIP_TRY(hipEventRecord(e_end, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    s->temporal_cur = to;
    s->temporal_camera = cam;
    s->temporal_has_camera = true;
    s->temporal_filled = true;
    if (ms_out) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, e_begin, e_end));
        *ms_out = (double)ms;
    }
    return SHM_OK;
}

int shm_temporal_read(ShmScene* s, ShmFilmPixel* out) {
    if (!s || !out) { shm_err() = "temporal: a null argument"; return SHM_ERR_INVALID_ARGUMENT; }
    if (!s->temporal_filled) { shm_err() = "temporal: nothing to read before shm_temporal_accumulate_device"; return SHM_ERR_INVALID_ARGUMENT; }
    return wf_read_pixels(s, s->d_temporal_out, sizeof(ShmFilmPixel), out);
}

int shm_temporal_read_history(ShmScene* s, ShmTemporalPixel* out) {
    if (!s || !out) { shm_err() = "temporal: a null argument"; return SHM_ERR_INVALID_ARGUMENT; }
    if (!s->temporal_filled) { shm_err() = "temporal: nothing to read before shm_temporal_accumulate_device"; return SHM_ERR_INVALID_ARGUMENT; }
    return wf_read_pixels(s, s->d_temporal[s->temporal_cur], sizeof(ShmTemporalPixel), out);
}

int shm_denoise_temporal_device(ShmScene* s, const ShmDenoiseParams* params, uint32_t temporal_variance, double* ms_out) {
    if (!s || !params) { shm_err() = "denoise: no scene or no parameters"; return SHM_ERR_INVALID_ARGUMENT; }
    if (!s->temporal_filled) { shm_err() = "denoise: no temporal result (no shm_temporal_accumulate_device since the scene was created or the history cleared)"; return SHM_ERR_INVALID_ARGUMENT; }
    if (params->variance_source != SHM_DENOISE_VARIANCE_SPATIAL) { shm_err() = "denoise: the temporal result is filtered with variance_source spatial only"; return SHM_ERR_INVALID_ARGUMENT; }
    if (temporal_variance > 1u) { shm_err() = "denoise: temporal_variance is 0 or 1"; return SHM_ERR_INVALID_ARGUMENT; }
    return wf_denoise_run(s, params, s->d_temporal_out, temporal_variance ? s->d_temporal[s->temporal_cur] : nullptr, ms_out);
}

}  // extern "C"
