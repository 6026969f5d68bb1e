// upe_rules.h — the rule compiler (upe_rules.cpp, plain C++: no GPU, any thread): what
// upe_gpu.hip installs into a context (struct upe_rule_image, build_image) and the neighbour
// snapshot upe_gpu_load_neigh uploads (NeighImage, build_neigh_image, with the cuckoo placement
// it shares with the compiler; struct upe_neigh_image).  The extern "C" entry points of the
// compiler (upe_rules_compile, upe_rules_image_free, upe_rules_match_host, upe_neigh_compile,
// upe_neigh_image_free) are in include/upe_gpu.h.
#ifndef UPE_RULES_H
#define UPE_RULES_H

#include <vector>

#include "../../include/upe_gpu.h"
#include "upe_dev.h"

namespace upe {

// Tuple-space index of one family of the compiled rules (see TssGroup).
struct TssFamily {
    std::vector<TssGroup> groups;
    std::vector<uint4> slots;
    std::vector<uint16_t> fp;   // one per slot
};

// Decision-tree index over the family lists (kTreeDims comment).
struct TreeImage {
    std::vector<uint2> nodes;
    std::vector<uint32_t> leaves;
    uint32_t trees[2] = {0, 0};      // trees per family
    uint32_t depth[2] = {0, 0};      // deepest leaf per family
    uint32_t max_leaf = 0;           // longest leaf list
    uint32_t swap6 = 0xFFu;          // IPv6 address words compared big-endian (tree_rule)
};

}  // namespace upe

// The compiled table a context classifies with (round 6: built apart from any context, so that
// a program's stats thread can build it while the workers keep forwarding, as the reference's
// does before its SIGHUP swap, src/main.c:222-257): the rule words, the family lists, the
// tuple-space index or the decision tree, and the flags the launches need.  Host memory only.
struct upe_rule_image {
    size_t count = 0, cap = 0, pad = 0;
    std::vector<upe::RuleV4> v4;
    std::vector<upe::RuleV6> v6;
    std::vector<int2> info;
    bool fwd4 = false, fwd6 = false;
    uint32_t fam4 = 0, fam6 = 0, fam_all = 0, fam_x1idx = 0;
    std::vector<uint4> fimg;
    bool tss = false;
    upe::TssFamily f4, f6;
    std::vector<uint16_t> fps;
    bool tree_ok = false;
    std::vector<uint4> timg;
    upe::TreeImage t;
    // (the type's name is the ABI's, upe_rule_image_t; its code is not exported)
    UPE_INTERNAL ~upe_rule_image() = default;
};

namespace upe {

// Compile a sorted table of `count` rules for a context whose rule_stats hold `cap` entries.
// 0, or -1 (upe_gpu_last_error()).
UPE_INTERNAL int build_image(const upe_rule_t* rules, size_t count, size_t cap, upe_rule_image& im);

// Three-choice cuckoo placement of the neighbour indexes' keys (slot1 / slot2 / slot3): starts at
// 2^bits >= 1.25 (n + room) slots, random-walk eviction, seeds tried, then doubles.  bits = 0 for
// no keys and no room; no keys with room: 2^bits free slots under the first seed.
// -1, at once, when more than three keys are equal (they share all three slots at every size).
UPE_INTERNAL int cuckoo3_place(const std::vector<uint32_t>& key, uint32_t& bits, uint32_t& seed,
                               std::vector<int32_t>& slot, size_t room = 0);

// The neighbour snapshot a context looks up in (NeighIndex, upe_gpu.hip): each family's slot
// array and its placement.  Host memory only; an empty family keeps one zero slot (bits 0).
struct UPE_INTERNAL NeighImage {
    std::vector<uint4> arp, ndp;
    uint32_t arp_bits = 0, arp_seed = 0, ndp_bits = 0, ndp_seed = 0;
    // For upe_gpu_neigh_learn, from the slot arrays compiled: their invalid slots, and whether
    // every valid slot is one a probe reaches and the index has slots (bits != 0).
    uint32_t arp_free = 0, ndp_free = 0;
    bool arp_insertable = false, ndp_insertable = false;
};

// Build the snapshot of the reference's slot arrays (power-of-two capacities, or 0): the entries
// a reference probe reaches, placed by cuckoo3_place with `room` more keys' worth of slots.  0, or
// -1 (upe_gpu_last_error()).
UPE_INTERNAL int build_neigh_image(const upe_arp_entry_t* arp, size_t arp_cap,
                                   const upe_ndp_entry_t* ndp, size_t ndp_cap, NeighImage& im,
                                   size_t arp_room = 0, size_t ndp_room = 0);

// upe_gpu_load_neigh's and upe_neigh_compile's arguments checked (power-of-two capacities of at
// most 2^30 slots, a table wherever there is a capacity, rooms of at most 2^30), then
// build_neigh_image.  0, or -1 (upe_gpu_last_error()).
UPE_INTERNAL int compile_neigh(const upe_arp_entry_t* arp, size_t arp_cap,
                               const upe_ndp_entry_t* ndp, size_t ndp_cap, NeighImage& im,
                               size_t arp_room = 0, size_t ndp_room = 0);

}  // namespace upe

// The compiled snapshot as the ABI hands it out (upe_neigh_compile): built apart from any
// context, as a upe_rule_image is, so that the thread that expires the neighbour tables can build
// it and a worker only uploads it (upe_gpu_load_neigh_image).  Host memory only.
// (the type's name is the ABI's, upe_neigh_image_t; its code is not exported)
struct UPE_INTERNAL upe_neigh_image {
    upe::NeighImage im;
};

#endif  // UPE_RULES_H
