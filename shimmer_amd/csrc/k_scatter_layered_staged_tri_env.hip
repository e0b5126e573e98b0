// k_scatter_layered_staged_tri_env.hip — k_scatter_layered_staged_tri.hip for scenes whose only image is an ImageInfinitelight (K_ENV_LIGHT; k_vertex_env.hip says why):
// the reference's showcase class — a coated object under an environment map.
#include "shm/fp.h"
#define SHM_BASE_BXDF_CALL SHM_HD_NOINLINE  // the walks call the interface BxDFs instead of inlining them ~30 times
#define K_ENV_LIGHT true
#include "k_scatter_layered.inl"

WF_SCATTER_LAYERED_STUB(GEO_TRI, IMG_ENV)
