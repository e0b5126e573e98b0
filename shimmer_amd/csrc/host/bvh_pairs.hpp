// host/bvh_pairs.hpp — the DEVICE layout of the BVH: sibling pairs, link words, the big leaves' counts, the instances' leaf slots and root records, as one pure
// function over a FlatScene (plain C++17, no HIP: oracle/oracle.cpp exports it to tests/test_bvh_pairs.py; render.hip uploads what it returns).
#pragma once
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../shm/bvh_link.h"
#include "flatten.h"

namespace shm_host {

struct BvhPairs {
    std::vector<ShmBvhNode> nodes;       // by sibling pairs, `offset` rewritten into the link word
    std::vector<uint32_t> big_leaf_n;    // n_prims left from each primitive slot on, only where a leaf holds LINK_COUNT_MAX primitives or more (empty otherwise)
    std::vector<ShmInstance> instances;  // root_node in the pair layout, pad[0] = the slot of the instance's leaf (0xffffffff: in no reachable leaf)
    std::vector<ShmBvhNode> inst_roots;  // each instance's root record
};

// The DEVICE copy of the tree is laid out by sibling pairs (the ABI's array and the oracle's stay in the reference's depth-first order,
// aggregate.rs:425-467): the two children of a node share one 64-byte block, the block of a node's first child's children follows. Depth first, a
// node's second child lies behind its sibling's whole subtree, and the fetch that a pop starts — the head of a dependent chain — misses; here it
// shares the block its sibling brought in. Same nodes, same visit order, same counters: an interior node's `offset` is its first child's index, the
// second child is offset + 1 (k_trace.hip). Headline frame: K2 136.0 -> 133.5 ms, K3 81.0 -> 77.8 ms (of which the larger-child-next order: 0.5 %).
inline int bvh_pairs(const FlatScene& f, BvhPairs& out, std::string& err) {
    using namespace wf;
    const std::vector<ShmBvhNode>& dn = f.nodes;
    out.instances = f.instances;
    for (ShmInstance& in : out.instances) in.pad[0] = 0xffffffffu;  // (the slot of the instance's leaf, filled in below; 0xffffffff: not seen yet)
    std::vector<uint32_t> new_index(dn.size(), 0xffffffffu);
    std::vector<uint32_t> roots{0u};
    for (const ShmInstance& in : f.instances) roots.push_back(in.root_node);
    std::sort(roots.begin(), roots.end());
    roots.erase(std::unique(roots.begin(), roots.end()), roots.end());
    uint32_t next = 0;
    std::vector<uint32_t> stack;
    for (uint32_t r : roots) {
        if (r >= dn.size()) { err = "instance root node out of range"; return SHM_ERR_INVALID_ARGUMENT; }
        // (a root inside another root's tree — an instanced SUB-tree — would get two device indices: named, not mis-traversed)
        if (new_index[r] != 0xffffffffu) { err = "an instance's root node lies inside another tree of the node array (instanced sub-trees are not supported: give the object its own tree)"; return SHM_ERR_INVALID_ARGUMENT; }
        new_index[r] = next;  // (a root sits alone in its block: the odd slot stays a zeroed, never-visited record)
        next += 2;
        stack.assign(1, r);
        while (!stack.empty()) {
            const uint32_t o = stack.back();
            stack.pop_back();
            if (dn[o].n_prims != 0) continue;
            const uint32_t c0 = o + 1u, c1 = dn[o].offset;
            if (c0 >= dn.size() || c1 >= dn.size() || new_index[c0] != 0xffffffffu || new_index[c1] != 0xffffffffu) {
                err = "BVH node array is not a depth-first tree"; return SHM_ERR_INVALID_ARGUMENT;
            }
            new_index[c0] = next;
            new_index[c1] = next + 1u;
            next += 2;
            // the child whose block of children comes next (and, half of the time, in the same 128-byte line): the one a ray is more likely to enter
            auto area = [&](const ShmBvhNode& n) {
                const float dx = n.bmax[0] - n.bmin[0], dy = n.bmax[1] - n.bmin[1], dz = n.bmax[2] - n.bmin[2];
                return dx * dy + dy * dz + dz * dx;
            };
            const bool first_next = !(area(dn[c1]) > area(dn[c0]));  // (the larger child's; "the first child's block next" measured 1 % slower in round 4)
            stack.push_back(first_next ? c1 : c0);
            stack.push_back(first_next ? c0 : c1);
        }
    }
    ShmBvhNode zero;
    memset(&zero, 0, sizeof(zero));
    out.nodes.assign(next, zero);
    out.big_leaf_n.clear();
    if (next > LINK_INDEX_MASK || f.prim_recs.size() > LINK_INDEX_MASK) { err = "more than 2^27 BVH nodes or primitives (the device link word holds 27-bit indices)"; return SHM_ERR_UNSUPPORTED; }
    for (size_t o = 0; o < dn.size(); ++o) {
        if (new_index[o] == 0xffffffffu) continue;  // (not reachable from any root)
        ShmBvhNode n = dn[o];
        // the link word (wavefront.h): where a traversal goes on from this node
        if (n.n_prims == 0) n.offset = ((uint32_t)n.axis << LINK_AXIS_SHIFT) | new_index[o + 1];
        else {
            if (n.n_prims >= LINK_COUNT_MAX) {
                if (out.big_leaf_n.empty()) out.big_leaf_n.assign(f.prim_recs.size(), 0u);
                for (uint32_t j = 0; j < n.n_prims; ++j) out.big_leaf_n[n.offset + j] = n.n_prims - j;  // (the primitives left from each slot on: k_trace5 takes one per phase)
            }
            // a leaf of ONE primitive that is no triangle is marked as such in the link word itself — a lane that reaches it parks for the wave's next round of
            // non-triangle work straight from the node step, without the leaf phase's fetch of a record it cannot test (k_trace5<., GEN>):
            //   an instance (always alone in its leaf, flatten.h): count 0, the INDEX of the instance in place of the slot (its slot rides in the device copy's pad[0]);
            //   a sphere / a bilinear patch: count 1 and the slot, as a lane would have parked on it
            const uint32_t kind1 = n.n_prims == 1 ? f.prim_recs[n.offset].kind_index : 0u;
            if (kind1 & shm::PRIM_INSTANCE_BIT) {
                const uint32_t idx = kind1 & shm::PRIM_INDEX_MASK;
                // (one leaf per ShmInstance: the traversal finds the instance's leaf slot — what a hit inside it is named by — in this record. Two instance primitives
                //  that shared one ShmInstance would overwrite each other's slot: refused, the host gives each primitive its own record)
                if (out.instances[idx].pad[0] != 0xffffffffu) { err = "two instance primitives share one ShmInstance record (give each TransformedPrimitive its own)"; return SHM_ERR_INVALID_ARGUMENT; }
                out.instances[idx].pad[0] = n.offset;
                n.offset = LINK_LEAF | LINK_OTHER | idx;
            } else if (kind1 & (shm::PRIM_SPHERE_BIT | shm::PRIM_PATCH_BIT)) {
                n.offset = LINK_LEAF | LINK_OTHER | (1u << LINK_COUNT_SHIFT) | n.offset;
            } else {
                n.offset = LINK_LEAF | (std::min<uint32_t>(n.n_prims, LINK_COUNT_MAX) << LINK_COUNT_SHIFT) | n.offset;
            }
        }
        out.nodes[new_index[o]] = n;
    }
    for (ShmInstance& in : out.instances) in.root_node = new_index[in.root_node];
    out.inst_roots.clear();
    for (const ShmInstance& in : out.instances) out.inst_roots.push_back(out.nodes[in.root_node]);
    return SHM_OK;
}

}  // namespace shm_host
