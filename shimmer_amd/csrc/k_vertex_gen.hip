// k_vertex_gen.hip — k_vertex for scenes with quadrics / bilinear patches / instances, no textures.
#include "k_vertex.inl"

WF_VERTEX_STUB(WF_VERTEX_LAUNCH, GEO_GEN, IMG_NONE)
