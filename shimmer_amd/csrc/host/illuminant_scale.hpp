// host/illuminant_scale.hpp — 1 / CIE Y of a densely sampled illuminant (471 entries, 360..=830): PBRT-v4's illumScale = 1 / SpectrumToY(illuminant), summed in double and
// rounded to float once. The ONE declaration: shm_scene_create (render.hip) keeps the float with the scene for the ambient occlusion integrator (shm/ao.h), and its CPU twin
// (host/host_mirror.cpp, shm_ao_samples_host) computes the same float. Defined in host/pbrt_loader.cpp, the unit that holds the CIE tables (host/spectral_tables.inc).
#pragma once
extern "C" __attribute__((visibility("hidden"))) float host_illuminant_scale(const float* illuminant);
