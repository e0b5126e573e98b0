// k_shade_lean.hip — the fused shade kernel of the one scene class that keeps it: triangles only, every material a DiffuseMaterial, no
// textures (the headline scene class). One BxDF class means there is nothing to sort, and the staged pipeline's parameter block would be
// pure HBM traffic; every other scene class runs k_vertex -> k_scatter<class> (k_vertex.inl, k_scatter.inl).
#include "k_shade.inl"

WF_SHADE_LEAN_STUBS(GEO_TRI, IMG_NONE)
