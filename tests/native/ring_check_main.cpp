// pv_ring.h against a brute-force walk of the fused kernel's hand-over ring, for every range size
// wt from 1 to 64 tiles: the four Net waves fill slots as net_fast_reg does (wave w's k-th tile is
// tile w + 4 k of the range; a wave past its last tile writes zeros), the inserting threads read
// them back as topn_combine does. Every tile of the range must arrive exactly once, at the record
// offset it has in the range, no slot may be written twice in a section, and every wave must count
// the same sections. Built with -fsanitize=address,undefined by tests/test_ring_index.py.
#include <cstdio>
#include <vector>
#define PV_FN inline
#include "../../pktvisor_amd/csrc/pv_ring.h"

int main()
{
    int bad = 0;
    for (uint32_t wt = 1; wt <= 64; wt++) {
        const uint32_t ns = pv_ring_sections(wt);
        // the fewest sections that hold the range
        if (ns * PV_RING_SLOTS < wt || (ns && (ns - 1) * PV_RING_SLOTS >= wt)) { printf("wt %u: %u sections\n", wt, ns); bad++; }
        // two sections of PV_RING_SLOTS slots: the tile a slot holds + 1, 0 for zeros
        std::vector<uint32_t> ring(2 * PV_RING_SLOTS);
        std::vector<uint32_t> seen(wt, 0);
        uint32_t secn = 0;
        for (uint32_t s = 0; s < ns; s++, secn++) {
            std::vector<uint32_t> wrote(PV_RING_SLOTS, 0);
            for (uint32_t w = 0; w < PV_RING_WAVES; w++) {
                const uint32_t ntl = wt > w ? (wt - w + PV_RING_WAVES - 1) / PV_RING_WAVES : 0; // the wave's own tiles
                // this turn of the wave's loop: k = s K .. s K + K - 1, the same turns in every wave
                for (uint32_t k = s * PV_RING_K; k < (s + 1) * PV_RING_K; k++) {
                    if (pv_ring_section(k) != s) { printf("wt %u: tile %u of wave %u in section %u\n", wt, k, w, pv_ring_section(k)); bad++; }
                    const uint32_t q = pv_ring_slot(w, k);
                    if (q >= PV_RING_SLOTS || wrote[q]++) { printf("wt %u: slot %u of section %u twice or out of range\n", wt, q, s); bad++; continue; }
                    ring.at((secn & 1) * PV_RING_SLOTS + q) = k < ntl ? w + PV_RING_WAVES * k + 1 : 0;
                }
            }
            for (uint32_t q = 0; q < PV_RING_SLOTS; q++) {
                const uint32_t v = ring.at((secn & 1) * PV_RING_SLOTS + q), t = pv_ring_tile(s, q);
                if (!v) {
                    if (t < wt) { printf("wt %u: tile %u missing\n", wt, t); bad++; }
                    continue;
                }
                if (v - 1 != t || t >= wt) { printf("wt %u: slot %u of section %u holds tile %u, read as %u\n", wt, q, s, v - 1, t); bad++; continue; }
                seen.at(t)++;
            }
        }
        for (uint32_t t = 0; t < wt; t++)
            if (seen[t] != 1) { printf("wt %u: tile %u inserted %u times\n", wt, t, seen[t]); bad++; }
    }
    printf("ring index check: %d errors\n", bad);
    return bad ? 1 : 0;
}
