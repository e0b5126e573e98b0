// k_generate_spherical.hip — K1 for a scene whose camera is PBRT-v4's spherical one (SHM_CAMERA_SPHERICAL): k_generate.inl once more, with the spherical branch of
// camera_generate_ray_differential (shm/path.h, SHM_SPHERICAL_CAMERA) compiled in. Its launcher is wf_generate<true> (wavefront.h); the render plan
// (host/render_plan.hpp, RenderPlan::spherical) names it for such a scene and for no other, so that every other scene runs render.hip's kernels,
// which are those of a library without this camera. A unit of its own: it compiles beside render.hip.
#define K_SPHERICAL_CAMERA true
#include "wavefront.h"
#include "k_generate.inl"
