// k_moments.hip — the moments pass's two kernels, its device entry points and the adaptive render loop on them (include/shimmer_hip.h,
// shm_moments_* and shm_render_adaptive). The arithmetic is shm/moments.h, which host/host_mirror.cpp compiles a second time for the CPU twin; the kernels here only
// say which pixels a lane owns and how a tile's two results leave the wave.
//   k_moments_clear    one pixel per lane: a zero record whose prev is the film pixel as it stands
//   k_moments_update   one 64-lane workgroup — one wave — per tile of the call's list. Lane l takes the tile's pixels l, l + 64, ... in row-major order: an 8x8 tile is
//                      one pixel per lane, a larger one is strode over, a clipped edge tile leaves lanes idle. Each lane updates its records from the film and evaluates
//                      `converged`; the tile's two results are order-free, so they are the same bits however the lanes are laid out: the count of unconverged pixels
//                      (a ballot's popcount per stride, the same sum in every lane) and the maximum e2 (a butterfly of six shuffles over an integer key whose
//                      order is the floats' total order). Lane 0 writes the ShmTileError with a vector store. No atomics, no floating-point sum across lanes, no LDS.
// The pass reads the film and writes only its own records: no render kernel knows of it. This unit draws no sample and shades nothing: it sets none of the shared
// headers' switches, and its name matches none of the Makefile's *_zs / *_dl patterns.
#include "wavefront.h"
#include "shm/moments.h"

namespace {

constexpr int MOM_WAVE = 64;
static_assert(sizeof(ShmFilmPixel) == 4 * sizeof(double) && sizeof(ShmMomentsPixel) == MOMENTS_DOUBLES * sizeof(double), "the pixel functions of shm/moments.h index film and record as doubles");
static_assert(sizeof(ShmTileError) == 8 && sizeof(ShmAdaptiveParams) == 32, "include/shimmer_hip.h: the adaptive structs' layout");

__global__ void __launch_bounds__(256) k_moments_clear(const ShmFilmPixel* film, ShmMomentsPixel* moments, uint32_t n) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    double f[4], m[MOMENTS_DOUBLES];
    for (int c = 0; c < 4; ++c) f[c] = reinterpret_cast<const double*>(film + q)[c];
    moments_clear_pixel(f, m);
    for (int c = 0; c < MOMENTS_DOUBLES; ++c) reinterpret_cast<double*>(moments + q)[c] = m[c];
}

__global__ void __launch_bounds__(MOM_WAVE) k_moments_update(const ShmFilmPixel* film, ShmMomentsPixel* moments, const ShmTile* tiles, int x_min, int y_min, int film_width,
                                                             MomentsConfig k, ShmTileError* out) {
    const ShmTile t = tiles[blockIdx.x];
    const int tw = t.x1 - t.x0, n = tw * (t.y1 - t.y0);  // (the host refused empty tiles and tiles outside the film)
    const int lane = (int)threadIdx.x;
    uint32_t unconverged = 0;
    uint32_t key = 0;  // below every float's key: a tile has a pixel, so some lane raises it
    for (int base = 0; base < n; base += MOM_WAVE) {  // (uniform: every lane reaches every ballot)
        const int i = base + lane;
        bool open = false;
        if (i < n) {
            const int x = t.x0 + i % tw, y = t.y0 + i / tw;
            const size_t q = (size_t)(y - y_min) * (size_t)film_width + (size_t)(x - x_min);
            double f[4], m[MOMENTS_DOUBLES];
            const double* fp = reinterpret_cast<const double*>(film + q);
            double* mp = reinterpret_cast<double*>(moments + q);
            for (int c = 0; c < 4; ++c) f[c] = fp[c];
            for (int c = 0; c < MOMENTS_DOUBLES; ++c) m[c] = mp[c];
            moments_update_pixel(f, m);
            for (int c = 0; c < MOMENTS_DOUBLES; ++c) mp[c] = m[c];
            const double e2 = moments_e2(m, k.mean_floor);
            open = !moments_converged(m, e2, k);
            const uint32_t ke = moments_key(moments_e2_float(e2));
            key = ke > key ? ke : key;
        }
        unconverged += (uint32_t)__popcll(__ballot(open));
    }
    for (int off = MOM_WAVE / 2; off > 0; off >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)key, off, MOM_WAVE);
        key = other > key ? other : key;
    }
    if (lane == 0) {
        ShmTileError e;
        e.unconverged = unconverged;
        e.max_e2 = moments_key_value(key);
        out[blockIdx.x] = e;
    }
}

MomentsConfig moments_config(const ShmAdaptiveParams& p) { return MomentsConfig{p.min_spp / p.batch_spp, p.threshold, p.floor}; }

// the pass's tile list and per-tile result on the device: one allocation, regrown when a call brings more tiles than any before
int ensure_tile_buffers(ShmScene* s, uint32_t n_tiles) {
    if (s->moments_tiles_capacity >= n_tiles) return SHM_OK;
    if (s->d_moments_tiles) {
        wf_scene_free(s, s->d_moments_tiles);
        s->d_moments_tiles = nullptr; s->d_tile_error = nullptr; s->moments_tiles_capacity = 0;
    }
    void* d = nullptr;
    if (wf_scene_alloc(s, (size_t)n_tiles * (sizeof(ShmTile) + sizeof(ShmTileError)), &d) != SHM_OK) { shm_err() = "hipMalloc of the moments pass's tile list failed"; return SHM_ERR_OUT_OF_MEMORY; }
    s->d_moments_tiles = reinterpret_cast<ShmTile*>(d);
    s->d_tile_error = reinterpret_cast<ShmTileError*>(s->d_moments_tiles + n_tiles);
    s->moments_tiles_capacity = n_tiles;
    return SHM_OK;
}

}  // namespace

extern "C" {

int shm_adaptive_default_params(ShmAdaptiveParams* out) {
    if (!out) return SHM_ERR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    out->min_spp = 16;
    out->batch_spp = 4;
    out->threshold = 0.05f;
    out->floor = 0.01f;
    return SHM_OK;
}

int shm_moments_clear(ShmScene* s) {
    if (!s) { shm_err() = "moments: no scene"; return SHM_ERR_INVALID_ARGUMENT; }
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = s->n_film_pixels;
    int rc;
    if (!s->d_moments && (rc = wf_scene_alloc(s, std::max<size_t>(n, 1) * sizeof(ShmMomentsPixel), (void**)&s->d_moments)) != SHM_OK) return rc;
    hipLaunchKernelGGL(k_moments_clear, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s->stream, s->d_film, s->d_moments, (uint32_t)n);
    LAUNCH_TRY("k_moments_clear");
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SHM_OK;
}

int shm_moments_update(ShmScene* s, const ShmTile* tiles, uint32_t n_tiles, const ShmAdaptiveParams* params, ShmTileError* out) {
    if (!s || !tiles || !params || !out || n_tiles == 0) { shm_err() = "moments: a null argument or no tiles"; return SHM_ERR_INVALID_ARGUMENT; }
    if (const char* why = moments_params_error(params->min_spp, params->batch_spp, params->threshold, params->floor)) { shm_err() = why; return SHM_ERR_INVALID_ARGUMENT; }
    if (!s->d_moments) { shm_err() = "moments: no shm_moments_clear on this scene yet"; return SHM_ERR_INVALID_ARGUMENT; }
    const int32_t* pb = s->flat.film.pixel_bounds;
    if (const char* why = moments_tiles_error(&tiles[0].x0, n_tiles, pb, s->tile_bitmap)) { shm_err() = why; return SHM_ERR_INVALID_ARGUMENT; }
    HIP_TRY(hipSetDevice(s->device));
    int rc;
    if ((rc = ensure_tile_buffers(s, n_tiles)) != SHM_OK) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_moments_tiles, tiles, (size_t)n_tiles * sizeof(ShmTile), hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_moments_update, dim3(n_tiles), dim3(MOM_WAVE), 0, s->stream, s->d_film, s->d_moments, s->d_moments_tiles, pb[0], pb[1], pb[2] - pb[0],
                       moments_config(*params), s->d_tile_error);
    LAUNCH_TRY("k_moments_update");
    HIP_TRY(hipMemcpyAsync(out, s->d_tile_error, (size_t)n_tiles * sizeof(ShmTileError), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    return SHM_OK;
}

int shm_moments_read(ShmScene* s, ShmMomentsPixel* out) {
    if (!s || !out) { shm_err() = "moments: a null argument"; return SHM_ERR_INVALID_ARGUMENT; }
    if (!s->d_moments) { shm_err() = "moments: no shm_moments_clear on this scene yet"; return SHM_ERR_INVALID_ARGUMENT; }
    return wf_read_pixels(s, s->d_moments, sizeof(ShmMomentsPixel), out);
}

int shm_render_adaptive(ShmScene* s, const ShmRenderParams* params, const ShmTile* tiles, uint32_t n_tiles, const ShmAdaptiveParams* ap, uint32_t* tile_spp_out,
                        ShmStats* stats) {
    if (!s || !params || !tiles || !ap || n_tiles == 0) { shm_err() = "adaptive: a null argument or no tiles"; return SHM_ERR_INVALID_ARGUMENT; }
    if (const char* why = moments_params_error(ap->min_spp, ap->batch_spp, ap->threshold, ap->floor)) { shm_err() = why; return SHM_ERR_INVALID_ARGUMENT; }
    const int cap = params->samples_per_pixel, batch = ap->batch_spp;
    if (cap < ap->min_spp) { shm_err() = "adaptive: samples_per_pixel (the cap) below min_spp"; return SHM_ERR_INVALID_ARGUMENT; }
    if (stats) memset(stats, 0, sizeof(*stats));
    int rc;
    if ((rc = shm_film_clear(s)) != SHM_OK) return rc;
    if ((rc = shm_moments_clear(s)) != SHM_OK) return rc;
    std::vector<ShmTileError> err(n_tiles);
    // the base batches: every tile, min_spp samples
    int spp = 0;
    for (; spp < ap->min_spp; spp += batch) {
        if ((rc = shm_render_wave(s, params, tiles, n_tiles, spp, spp + batch, stats)) != SHM_OK) return rc;
        if ((rc = shm_moments_update(s, tiles, n_tiles, ap, err.data())) != SHM_OK) return rc;
    }
    std::vector<uint32_t> tile_spp(n_tiles, (uint32_t)spp);
    // the refinement rounds: `active` only shrinks, so its tiles share one spp
    std::vector<uint32_t> active(n_tiles), next;
    for (uint32_t i = 0; i < n_tiles; ++i) active[i] = i;
    std::vector<ShmTile> sub;
    while (spp < cap) {
        next.clear();
        for (size_t j = 0; j < active.size(); ++j)
            if (err[j].unconverged > 0) next.push_back(active[j]);
        active.swap(next);
        if (active.empty()) break;
        sub.resize(active.size());
        for (size_t j = 0; j < active.size(); ++j) sub[j] = tiles[active[j]];
        const int end = std::min(spp + batch, cap);
        if ((rc = shm_render_wave(s, params, sub.data(), (uint32_t)sub.size(), spp, end, stats)) != SHM_OK) return rc;
        if ((rc = shm_moments_update(s, sub.data(), (uint32_t)sub.size(), ap, err.data())) != SHM_OK) return rc;
        spp = end;
        for (uint32_t i : active) tile_spp[i] = (uint32_t)spp;
    }
    if (tile_spp_out) memcpy(tile_spp_out, tile_spp.data(), (size_t)n_tiles * sizeof(uint32_t));
    return SHM_OK;
}

}  // extern "C"
