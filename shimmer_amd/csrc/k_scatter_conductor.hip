// k_scatter_conductor.hip — the scattering half of a vertex (k_scatter.inl) for the CLASS_CONDUCTOR queue, in the three scene classes.
#include "k_scatter.inl"

WF_SCATTER_STUB(FAM_SCATTER_CONDUCTOR, GEO_GEN, IMG_TEX)
WF_SCATTER_STUB(FAM_SCATTER_CONDUCTOR, GEO_TRI, IMG_NONE)
WF_SCATTER_STUB(FAM_SCATTER_CONDUCTOR, GEO_GEN, IMG_NONE)
