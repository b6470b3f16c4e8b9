// SPDX-License-Identifier: MPL-2.0
//
// pv_geo.hip — device walker of a compiled GeoIP / ASN search tree (pv_geodb.h): the lookup of
// MMDB_lookup_sockaddr (libmaxminddb's find_address_in_search_tree) over the uniform tree.
//
// One lane an address. A node is two uint32 words (bit 0, bit 1); a word below node_count is the
// next node, any other is a leaf (PV_GEO_LEAF | dictionary id). The loop ends at the address's
// bit count (32 / 128) or at the first word that is not a node, so it cannot spin and cannot
// index past the tree whatever the words hold. The loads of one walk depend on each other; lanes
// hide each other's latency, and the first levels of the tree stay in L2.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pv_geodb.h"

extern "C" __global__ void __launch_bounds__(256)
pv_geo_walk(const uint32_t *__restrict__ tree, uint32_t node_count, uint32_t start, const uint32_t *__restrict__ addrs,
            uint64_t n, uint32_t addr_words, uint32_t *__restrict__ ids)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t *a = addrs + i * addr_words;
        uint32_t w = start;
        for (uint32_t k = 0; k < addr_words; k++) w = pv_geo_step32(tree, node_count, w, __builtin_bswap32(a[k])); // network order
        ids[i] = pv_geo_id(w);
    }
}
