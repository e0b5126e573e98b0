// k_shade_lean_gen_env.hip — k_shade_lean_env.hip for scenes that hold spheres, bilinear patches or instances: k_shade.inl <false, TRI_ONLY = false, false, true, false, false,
// ENV_LIGHT = true>.
#include "k_shade.inl"

WF_SHADE_LEAN_STUBS(GEO_GEN, IMG_ENV)
