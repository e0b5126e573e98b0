// k_shade_lean_prefetch.hip — k_shade_lean.hip's kernel once more, as the instantiation that fetches a lane's next vertex while it shades this one (k_shade.inl:
// K_SHADE_PREFETCH; the renders with compact hit records run it). A unit of its own: beside the plain instantiation in one unit both kernels spill.
#include "k_shade.inl"

WF_SHADE_LEAN_PREFETCH_STUB()
