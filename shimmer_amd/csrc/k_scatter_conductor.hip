// k_scatter_conductor.hip — the scattering half of a vertex (k_scatter.inl) for the CLASS_CONDUCTOR queue, in the three scene classes.
#include "k_scatter.inl"

template <> int wf_launch_scatter_conductor_tex<K_ZSOBOL, K_DELTA_LIGHTS>(ShmScene* s, const ShadeArgs& a) { WF_SCATTER_LAUNCH(CLASS_CONDUCTOR, false, true); return SHM_OK; }
template <> int wf_launch_scatter_conductor_tri<K_ZSOBOL, K_DELTA_LIGHTS>(ShmScene* s, const ShadeArgs& a) { WF_SCATTER_LAUNCH(CLASS_CONDUCTOR, true, false); return SHM_OK; }
template <> int wf_launch_scatter_conductor_gen<K_ZSOBOL, K_DELTA_LIGHTS>(ShmScene* s, const ShadeArgs& a) { WF_SCATTER_LAUNCH(CLASS_CONDUCTOR, false, false); return SHM_OK; }
