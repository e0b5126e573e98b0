// k_vertex_tex.hip — k_vertex for scenes that bind image textures or an image infinite light (ray differentials, MIP filtering).
#include "k_vertex.inl"

WF_VERTEX_STUB(WF_VERTEX_LAUNCH, GEO_GEN, IMG_TEX)
