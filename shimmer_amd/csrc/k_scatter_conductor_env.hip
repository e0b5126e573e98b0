// k_scatter_conductor_env.hip — k_scatter_conductor.hip for scenes whose only image is an ImageInfinitelight (K_ENV_LIGHT, k_scatter.inl; k_vertex_env.hip says why).
#define K_ENV_LIGHT true
#include "k_scatter.inl"

WF_SCATTER_STUB(FAM_SCATTER_CONDUCTOR, GEO_TRI, IMG_ENV)
WF_SCATTER_STUB(FAM_SCATTER_CONDUCTOR, GEO_GEN, IMG_ENV)
