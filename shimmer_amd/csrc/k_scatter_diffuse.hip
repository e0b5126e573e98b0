// k_scatter_diffuse.hip — the scattering half of a vertex (k_scatter.inl) for the CLASS_DIFFUSE queue, in the three scene classes.
#include "k_scatter.inl"

template <> int wf_launch_scatter_diffuse_tex<K_ZSOBOL, K_DELTA_LIGHTS>(ShmScene* s, const ShadeArgs& a) { WF_SCATTER_LAUNCH(CLASS_DIFFUSE, false, true); return SHM_OK; }
template <> int wf_launch_scatter_diffuse_tri<K_ZSOBOL, K_DELTA_LIGHTS>(ShmScene* s, const ShadeArgs& a) { WF_SCATTER_LAUNCH(CLASS_DIFFUSE, true, false); return SHM_OK; }
template <> int wf_launch_scatter_diffuse_gen<K_ZSOBOL, K_DELTA_LIGHTS>(ShmScene* s, const ShadeArgs& a) { WF_SCATTER_LAUNCH(CLASS_DIFFUSE, false, false); return SHM_OK; }
