// k_scatter_conductor_env.hip — k_scatter_conductor.hip for scenes whose only image is an ImageInfinitelight (K_ENV_LIGHT, k_scatter.inl; k_vertex_env.hip says why).
#define K_ENV_LIGHT true
#include "k_scatter.inl"

template <> int wf_launch_scatter_conductor_tri_env<K_ZSOBOL, K_DELTA_LIGHTS>(ShmScene* s, const ShadeArgs& a) { WF_SCATTER_LAUNCH(CLASS_CONDUCTOR, true, false); return SHM_OK; }
template <> int wf_launch_scatter_conductor_gen_env<K_ZSOBOL, K_DELTA_LIGHTS>(ShmScene* s, const ShadeArgs& a) { WF_SCATTER_LAUNCH(CLASS_CONDUCTOR, false, false); return SHM_OK; }
