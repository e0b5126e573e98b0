// shm/bvh_link.h — the link word of a DEVICE BVH node (wavefront.h, "The DEVICE copy of a BVH node"): host/bvh_pairs.hpp writes it, k_trace.hip reads it.
#pragma once
#include <stdint.h>
namespace wf {
constexpr uint32_t LINK_LEAF = 0x80000000u, LINK_OTHER = 0x40000000u, LINK_INDEX_MASK = 0x07ffffffu, LINK_COUNT_SHIFT = 27u, LINK_COUNT_MAX = 7u, LINK_AXIS_SHIFT = 29u;
}  // namespace wf
