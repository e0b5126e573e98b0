// k_vertex_tri.hip — k_vertex for scenes made of top-level triangles only, no textures.
#include "k_vertex.inl"

// 159 VGPRs: three waves per SIMD hide the latency of the hit / vertex gathers (measured on C4 against the two-wave build: k_vertex 142 -> 110 ms per frame).
WF_VERTEX_STUB(WF_VERTEX_LAUNCH_W3, GEO_TRI, IMG_NONE)
