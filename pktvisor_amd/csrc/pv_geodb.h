// SPDX-License-Identifier: MPL-2.0
//
// pv_geodb.h — host reader of MaxMind DB (format 2.0) files, compiled at open time into the
// form the device walker reads. Plain C++, no HIP: the reader works on a machine without a GPU.
//
// Replaces the MaxmindDB wrapper of the reference (src/GeoDB.h:27-41, src/GeoDB.cpp): instead of
// decoding the data record of every lookup, every data record the search tree can reach is
// decoded once at open time and rendered to the string the handlers count by
// (_getGeoLoc, GeoDB.cpp:179-244; _getASNString, :371-413). Equal strings share one dense id;
// id 0 is the "Unknown" of a lookup that finds no entry.
#ifndef PV_GEODB_H
#define PV_GEODB_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#define PV_GEO_LEAF 0x80000000u // a tree word with this bit carries a dictionary id, not a node
#define PV_GEO_MAX_DEPTH 32     // nesting of maps / arrays the decoder follows

#ifdef __HIPCC__
#define PV_GEO_HD __host__ __device__
#else
#define PV_GEO_HD
#endif
// The walk, 32 address bits at a time (first bit = the top one): from word w along `bits` until
// a word is not a node. The host lookup, pv_geo_walk and pv_geo_count all walk with this; the
// condition keeps every index below node_count whatever the tree holds.
PV_GEO_HD inline uint32_t pv_geo_step32(const uint32_t *tree, uint32_t node_count, uint32_t w, uint32_t bits)
{
    for (int b = 31; b >= 0 && w < node_count; b--) w = tree[(uint64_t)w * 2 + ((bits >> b) & 1u)];
    return w;
}
// a finished walk's dictionary id (a word still a node after the last bit: no entry)
PV_GEO_HD inline uint32_t pv_geo_id(uint32_t w) { return (w & PV_GEO_LEAF) ? (w & ~PV_GEO_LEAF) : 0u; }

// pv_geo_count's view of the attached databases ([0] city, [1] ASN; tree == nullptr: not attached)
struct PvGeoArgs {
    const uint32_t *tree[2];
    unsigned long long *cnt[2]; // PV_SLOTS x entries: packets per Net slot and dictionary id
    // Net v2 (pv_set_v2_geo): PV_SLOTS x 3 x entries, packets per Net slot, direction and dictionary
    // id; null: the v2 handler does not count. (cnt is null likewise while v1's top_geo is off.)
    unsigned long long *cnt2[2];
    uint32_t node_count[2], start4[2], ip_version[2], entries[2];
};

struct pv_geodb {
    uint32_t kind = 0;       // PV_GEODB_CITY / PV_GEODB_ASN
    uint32_t ip_version = 0; // 4 or 6
    uint32_t node_count = 0;
    // Uniform tree: two words a node (bit 0, bit 1). A word below node_count is the next node
    // (validated), any other has PV_GEO_LEAF set and carries a dictionary id.
    std::vector<uint32_t> tree;
    uint32_t start4 = PV_GEO_LEAF; // where an IPv4 walk starts: the root, or what 96 zero bits of
                                   // an ip_version 6 tree reach (may already be a leaf)
    struct Entry {
        std::string name, lat, lon; // City: location, latitude, longitude; ASN: the string, "", ""
    };
    std::vector<Entry> dict; // dict[0] = {"Unknown", "", ""}
    uint64_t hash = 0;       // FNV-1a of the tree and the dictionary: ranks compare it
};

namespace pvgeo {
// Parse and compile; nullptr and a message in err for a file that is not a well-formed database.
pv_geodb *open(const uint8_t *buf, size_t len, uint32_t kind, std::string &err);
// The walk of the compiled tree: addr_len 4 or 16 (network order). Bounded by the address bits.
uint32_t lookup(const pv_geodb &db, const uint8_t *addr, uint32_t addr_len);
} // namespace pvgeo

#endif
