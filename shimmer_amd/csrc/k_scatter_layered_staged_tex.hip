// k_scatter_layered_staged_tex.hip — the LayeredBxDF queue's scattering half as dense per-wave stages (k_scatter_layered.inl). Scene class <TRI_ONLY, HAS_TEX> = <false,true>.
#include "shm/fp.h"
#define SHM_BASE_BXDF_CALL SHM_HD_NOINLINE  // the walks call the interface BxDFs instead of inlining them ~30 times
#include "k_scatter_layered.inl"

WF_SCATTER_LAYERED_STUB(GEO_GEN, IMG_TEX)
