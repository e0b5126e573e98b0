// k_shade_lean_env.hip — the lean fused kernel (k_shade_lean.hip, k_shade_lean_gen.hip) for all-diffuse scenes whose only image is an ImageInfinitelight (round 5):
// k_shade.inl <HAS_LAYERED = false, TRI_ONLY, HAS_TEX = false, DIFFUSE_ONLY = true, EMIT_INLINE = false, SORT_CHUNK = false, ENV_LIGHT = true>. Until then an environment
// map put a scene into the textured class — ray differentials, auxiliary rays, the texture evaluators' registers — although nothing in it filters a texture: the object of
// the headline scene under a map ran at 2.9 Gray/s against 5.1 in its room. The light's look-up, sample and pdf are the shared functions of shm/path.h / shm/texture.h.
#include "k_shade.inl"

WF_SHADE_LEAN_STUBS(GEO_TRI, IMG_ENV)
