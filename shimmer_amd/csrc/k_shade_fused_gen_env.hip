// k_shade_fused_gen_env.hip — k_shade_tail_sorted_env.hip for scenes that hold spheres, bilinear patches or instances: k_shade.inl <false, TRI_ONLY = false, false, false, true,
// SORT_CHUNK = true, ENV_LIGHT = true>.
#ifndef K_SHADE_LEAN_WAVES
#define K_SHADE_LEAN_WAVES 2
#endif
#include "k_shade.inl"

WF_SHADE_FUSED_ALL_STUB(GEO_GEN, IMG_ENV)
