// k_denoise.hip — the denoiser's five kernels and its device entry points (include/shimmer_hip.h, shm_denoise_*). The arithmetic is shm/denoise.h,
// which host/host_mirror.cpp compiles a second time for the CPU twin; the kernels here only say which pixel a lane owns and where its taps come from.
//   k_denoise_prepare    one pixel per lane: the film's and the G-buffer's double sums -> planes A (e.rgb, var), B (n.xyz, l), C (p.xyz, valid), D (a_eff.rgb)
//   k_denoise_variance   one pixel per lane: the 7x7 moments of l -> A.w
//   k_denoise_variance_measured   one pixel per lane, after k_denoise_variance where ShmDenoiseParams::variance_source asks: the moments pass's measured variance over A.w
//                        at every valid pixel whose record holds two batches or more (DESIGN.md section 4k's v)
//   k_denoise_atrous     one launch per iteration, A -> A' (ping-pong): a workgroup owns a 32x8 block of ONE of the step^2 decimated sub-lattices, on which the a-trous
//                        filter is a dense 5x5 one. It stages the block's 36x12 halo tile of A, B and C into LDS (20.25 KiB) and every tap is a 16-byte LDS read — the
//                        same body at every step. (The plain gather — adjacent pixels per block, every tap from global memory — was built and measured against it and
//                        lost at every step: profiles/denoise.md.)
//   k_denoise_finish     one pixel per lane: e a_eff, or c for a pass-through pixel, as a ShmFilmPixel
// The launches are wf_denoise_run's: shm_denoise_device runs it over the scene's film, shm_denoise_temporal_device (k_temporal.hip) over the temporal pass's result, with
// that unit's k_temporal_variance behind the variance pass. The kernels do not know which.
// A workgroup is 32 lanes wide so that each of ds_read_b128's 16-lane groups (lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} of a half wave) lies in ONE tile row and
// reads 16 different 16-byte slots modulo 16: conflict-free whatever the tile's pitch. (A 16-wide block puts a group on two rows, and the pitch of 20 a 16x16 block's halo
// tile has then lands lanes 12-15 of one row on the slots of lanes 20-23 of the next.)
// This unit draws no sample and shades nothing: it sets none of the shared headers' switches, and its name matches none of the Makefile's *_zs / *_dl patterns.
#include "wavefront.h"
#include "shm/denoise.h"

namespace {

constexpr int DN_TX = 32, DN_TY = 8, DN_BLOCK = DN_TX * DN_TY;
constexpr int DN_HALO = 2, DN_PITCH = DN_TX + 2 * DN_HALO, DN_ROWS = DN_TY + 2 * DN_HALO;
static_assert(sizeof(ShmFilmPixel) == 4 * sizeof(double) && sizeof(ShmGBufferPixel) == 16 * sizeof(double), "the pixel functions of shm/denoise.h index the sums as doubles");
static_assert(sizeof(DnF4) == sizeof(float4), "a plane entry is a float4");
static_assert(sizeof(ShmMomentsPixel) == MOMENTS_DOUBLES * sizeof(double), "denoise_measured_variance indexes the record as doubles");

__global__ void __launch_bounds__(DN_BLOCK) k_denoise_prepare(const ShmFilmPixel* film, const ShmGBufferPixel* gbuffer, uint32_t n, float white_r, float white_g, float white_b,
                                                              DenoiseConfig k, DnF4* A, DnF4* B, DnF4* C, DnF4* D) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float white[3] = {white_r, white_g, white_b};
    DnF4 a, b, c, d;
    denoise_prepare_pixel(reinterpret_cast<const double*>(film + q), reinterpret_cast<const double*>(gbuffer + q), white, k, a, b, c, d);
    A[q] = a; B[q] = b; C[q] = c; D[q] = d;
}

__global__ void __launch_bounds__(DN_BLOCK) k_denoise_variance(DnF4* A, const DnF4* B, const DnF4* C, int width, int height, DenoiseConfig k) {
    const int x = (int)(blockIdx.x * DN_TX + threadIdx.x % DN_TX), y = (int)(blockIdx.y * DN_TY + threadIdx.x / DN_TX);
    if (x >= width || y >= height) return;
    const DenoiseGlobalTaps taps{nullptr, B, C, x, y, width, height, 1, false};
    // (the pass reads planes B and C only — DenoiseGlobalTaps::guides — and writes A.w alone)
    A[(size_t)y * (size_t)width + (size_t)x].w = denoise_variance_pixel(taps, k);
}

__global__ void __launch_bounds__(DN_BLOCK) k_denoise_variance_measured(DnF4* A, const DnF4* C, const DnF4* D, const ShmMomentsPixel* moments, uint32_t n) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n || C[q].w == 0.0f) return;
    const double* m = reinterpret_cast<const double*>(moments + q);
    if (!(m[11] >= 2.0)) return;  // fewer than two batches: the spatial estimate stays
    A[q].w = denoise_measured_variance(m, D[q]);
}

// The LDS tile of one sub-lattice block as denoise_atrous_pixel's window: tap (i, j) is the tile entry (i, j) away; an entry outside the film was staged with valid = 0.
struct DenoiseTileTaps {
    const DnF4 *A, *B, *C;  // at the pixel's own entry
    __device__ bool tap(int i, int j, DnF4& a, DnF4& b, DnF4& c) const {
        const int o = j * DN_PITCH + i;
        c = C[o];
        if (c.w == 0.0f) return false;
        a = A[o];
        b = B[o];
        return true;
    }
};  // (no guides(): the variance pass reads global memory)

__global__ void __launch_bounds__(DN_BLOCK) k_denoise_atrous(const DnF4* A, const DnF4* B, const DnF4* C, DnF4* A_out, int width, int height, int step, DenoiseConfig k) {
    const int tx = (int)threadIdx.x % DN_TX, ty = (int)threadIdx.x / DN_TX;
    __shared__ DnF4 s_a[DN_ROWS * DN_PITCH], s_b[DN_ROWS * DN_PITCH], s_c[DN_ROWS * DN_PITCH];
    // sub-lattice (ox, oy): the pixels (ox + step u, oy + step v); this block owns u in [u0, u0 + 32), v in [v0, v0 + 8)
    const int ox = (int)blockIdx.z % step, oy = (int)blockIdx.z / step;
    const int u0 = (int)blockIdx.x * DN_TX, v0 = (int)blockIdx.y * DN_TY;
    if (ox + step * u0 >= width || oy + step * v0 >= height) return;  // (the grid is sized for sub-lattice (0, 0), the largest; the whole block leaves)
    for (int t = (int)threadIdx.x; t < DN_ROWS * DN_PITCH; t += DN_BLOCK) {
        const int u = u0 - DN_HALO + t % DN_PITCH, v = v0 - DN_HALO + t / DN_PITCH;
        const int qx = ox + step * u, qy = oy + step * v;
        DnF4 a = dn_f4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a;
        if (u >= 0 && v >= 0 && qx < width && qy < height) {
            const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
            c = C[q];
            if (c.w != 0.0f) {
                a = A[q];
                b = B[q];
                b.w = denoise_luminance(a);  // l of the iteration's input, once per staged pixel
            }
        }
        s_a[t] = a; s_b[t] = b; s_c[t] = c;
    }
    __syncthreads();
    const int x = ox + step * (u0 + tx), y = oy + step * (v0 + ty);
    if (x >= width || y >= height) return;
    const int o = (ty + DN_HALO) * DN_PITCH + tx + DN_HALO;
    const DenoiseTileTaps taps{s_a + o, s_b + o, s_c + o};
    A_out[(size_t)y * (size_t)width + (size_t)x] = denoise_atrous_pixel(taps, k);
}

__global__ void __launch_bounds__(DN_BLOCK) k_denoise_finish(const ShmFilmPixel* film, uint32_t n, const DnF4* A, const DnF4* C, const DnF4* D, int filtered, ShmFilmPixel* out) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    DnF4 a = dn_f4(0.0f, 0.0f, 0.0f, 0.0f), d = a;
    bool valid = false;
    if (filtered && C[q].w != 0.0f) { valid = true; a = A[q]; d = D[q]; }
    double o[4];
    denoise_finish_pixel(reinterpret_cast<const double*>(film + q), valid, a, d, o);
    out[q].rgb_sum[0] = o[0]; out[q].rgb_sum[1] = o[1]; out[q].rgb_sum[2] = o[2]; out[q].weight_sum = o[3];
}

}  // namespace

// shm_denoise_device's body (wavefront.h): `film` is the scene's film or a ShmFilmPixel array that stands in for it
int wf_denoise_run(ShmScene* s, const ShmDenoiseParams* params, const ShmFilmPixel* film, const float4* temporal_records, double* ms_out) {
    const DenoiseConfig k{params->iterations, params->demodulate, params->sigma_luminance, params->sigma_normal, params->sigma_plane, params->albedo_floor};
    if (const char* why = denoise_params_error(k)) { shm_err() = why; return SHM_ERR_INVALID_ARGUMENT; }
    if (params->variance_source > SHM_DENOISE_VARIANCE_MEASURED) { shm_err() = "denoise: unknown variance_source"; return SHM_ERR_INVALID_ARGUMENT; }
    const bool measured = params->variance_source == SHM_DENOISE_VARIANCE_MEASURED;
    if (measured && !s->d_moments) { shm_err() = "denoise: variance_source is measured, but the scene has no moments (no shm_moments_clear yet)"; return SHM_ERR_INVALID_ARGUMENT; }
    if (!s->d_gbuffer || !s->gbuffer_filled) {
        shm_err() = "denoise: the scene's G-buffer is empty (no shm_gbuffer_render_wave / shm_render_gbuffer since the scene was created or the G-buffer cleared)";
        return SHM_ERR_INVALID_ARGUMENT;
    }
    HIP_TRY(hipSetDevice(s->device));
    const size_t n = s->n_film_pixels;
    if (!s->d_denoise) {  // planes A, A', B, C, D, then the result: one allocation, the scene's to free
        int rc;
        if ((rc = wf_scene_alloc(s, std::max<size_t>(n, 1) * (5 * sizeof(float4) + sizeof(ShmFilmPixel)), (void**)&s->d_denoise)) != SHM_OK) return rc;
        s->d_denoised = reinterpret_cast<ShmFilmPixel*>(s->d_denoise + 5 * std::max<size_t>(n, 1));
    }
    const int32_t* pb = s->flat.film.pixel_bounds;
    const int width = pb[2] - pb[0], height = pb[3] - pb[1];
    DnF4* planes = reinterpret_cast<DnF4*>(s->d_denoise);
    DnF4* A[2] = {planes, planes + n};
    DnF4 *B = planes + 2 * n, *C = planes + 3 * n, *D = planes + 4 * n;
    double white[3] = {0.0, 0.0, 0.0};  // shm_gbuffer_white
    const std::vector<float>* tables[3] = {&s->flat.sensor_r, &s->flat.sensor_g, &s->flat.sensor_b};
    for (int c = 0; c < 3; ++c)
        for (float v : *tables[c]) white[c] += (double)v;
    EventPool ev{s};
    hipEvent_t e_begin = ev.get(), e_end = ev.get();
    if (ev.failed) { shm_err() = "hipEventCreate failed"; return SHM_ERR_DEVICE; }
    const dim3 block(DN_BLOCK), linear((unsigned)((n + DN_BLOCK - 1) / DN_BLOCK)), tiles((unsigned)((width + DN_TX - 1) / DN_TX), (unsigned)((height + DN_TY - 1) / DN_TY));
    HIP_TRY(hipEventRecord(e_begin, s->stream));
    int cur = 0;
    if (k.iterations > 0) {
        hipLaunchKernelGGL(k_denoise_prepare, linear, block, 0, s->stream, film, s->d_gbuffer, (uint32_t)n, (float)white[0], (float)white[1], (float)white[2], k, A[0], B, C, D);
        LAUNCH_TRY("k_denoise_prepare");
        if (!is_inf(k.sigma_luminance)) {  // (nothing reads the variance otherwise but the next iteration's own)
            hipLaunchKernelGGL(k_denoise_variance, tiles, block, 0, s->stream, A[0], B, C, width, height, k);
            LAUNCH_TRY("k_denoise_variance");
            if (measured) {
                hipLaunchKernelGGL(k_denoise_variance_measured, linear, block, 0, s->stream, A[0], C, D, s->d_moments, (uint32_t)n);
                LAUNCH_TRY("k_denoise_variance_measured");
            }
            if (temporal_records) {
                int rc;
                if ((rc = wf_launch_temporal_variance(s->stream, reinterpret_cast<float4*>(A[0]), reinterpret_cast<const float4*>(C), temporal_records, (uint32_t)n)) != SHM_OK) return rc;
            }
        }
        for (uint32_t i = 0; i < k.iterations; ++i, cur ^= 1) {
            const int step = 1 << i;
            // the grid covers sub-lattice (0, 0), the largest, once per sub-lattice (blockIdx.z)
            const int sub_w = (width + step - 1) / step, sub_h = (height + step - 1) / step;
            const dim3 grid((unsigned)((sub_w + DN_TX - 1) / DN_TX), (unsigned)((sub_h + DN_TY - 1) / DN_TY), (unsigned)(step * step));
            hipLaunchKernelGGL(k_denoise_atrous, grid, block, 0, s->stream, A[cur], B, C, A[cur ^ 1], width, height, step, k);
            LAUNCH_TRY("k_denoise_atrous");
        }
    }
    hipLaunchKernelGGL(k_denoise_finish, linear, block, 0, s->stream, film, (uint32_t)n, A[cur], C, D, k.iterations > 0 ? 1 : 0, s->d_denoised);
    LAUNCH_TRY("k_denoise_finish");
    HIP_TRY(hipEventRecord(e_end, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipGetLastError());
    s->denoised = true;
    if (ms_out) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, e_begin, e_end));
        *ms_out = (double)ms;
    }
    return SHM_OK;
}

extern "C" {

int shm_denoise_default_params(ShmDenoiseParams* out) {
    if (!out) return SHM_ERR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    out->iterations = 5;
    out->demodulate = 1;
    out->sigma_luminance = 1.5f;
    out->sigma_normal = 128.0f;
    out->sigma_plane = 0.1f;
    out->albedo_floor = 0.01f;
    return SHM_OK;
}

int shm_denoise_device(ShmScene* s, const ShmDenoiseParams* params, double* ms_out) {
    if (!s || !params) { shm_err() = "denoise: no scene or no parameters"; return SHM_ERR_INVALID_ARGUMENT; }
    return wf_denoise_run(s, params, s->d_film, nullptr, ms_out);
}

int shm_denoise_read(ShmScene* s, ShmFilmPixel* out) {
    if (!s || !out) return SHM_ERR_INVALID_ARGUMENT;
    if (!s->denoised) { shm_err() = "denoise: nothing to read before shm_denoise_device"; return SHM_ERR_INVALID_ARGUMENT; }
    return wf_read_pixels(s, s->d_denoised, sizeof(ShmFilmPixel), out);
}

int shm_denoise(ShmScene* s, const ShmDenoiseParams* params, ShmFilmPixel* out, double* ms_out) {
    if (!out) return SHM_ERR_INVALID_ARGUMENT;
    const int rc = shm_denoise_device(s, params, ms_out);
    return rc != SHM_OK ? rc : shm_denoise_read(s, out);
}

}  // extern "C"
