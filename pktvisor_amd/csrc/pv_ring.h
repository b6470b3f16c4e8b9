// pv_ring.h: index arithmetic of pv_net_combine_ring's hand-over ring (pv_kernels.hip). The four
// Net waves of a workgroup take tiles w, w + 4, ... of a range (wave w's k-th tile is tile w + 4 k);
// a section of the ring holds PV_RING_K consecutive tiles of each wave, slot w * PV_RING_K + k %
// PV_RING_K. Every wave of the workgroup meets one barrier a section, so the section count of a
// range comes from the range's tile count alone, never from a wave's own.
// The includer defines PV_FN (device: __device__ __forceinline__, host tests: inline).
#pragma once
#include <stdint.h>

#define PV_RING_WAVES 4 // Net waves of the fused workgroup
#define PV_RING_K 3     // tiles of each Net wave a section: the depth of the Net pass's load pipeline
#define PV_RING_SLOTS (PV_RING_WAVES * PV_RING_K)

// sections (and barriers) of a range of `tiles` tiles: wave 0 has the most tiles, ceil(tiles / 4)
PV_FN uint32_t pv_ring_sections(uint32_t tiles)
{
    return (tiles + PV_RING_SLOTS - 1) / PV_RING_SLOTS;
}
// wave w's k-th tile: its section of the range and its slot there
PV_FN uint32_t pv_ring_section(uint32_t k) { return k / PV_RING_K; }
PV_FN uint32_t pv_ring_slot(uint32_t w, uint32_t k) { return w * PV_RING_K + k % PV_RING_K; }
// the range's tile that slot `slot` of the range's section `sec` holds (it may lie past the
// range's last tile: the slot then holds zeros)
PV_FN uint32_t pv_ring_tile(uint32_t sec, uint32_t slot)
{
    return slot / PV_RING_K + PV_RING_WAVES * (sec * PV_RING_K + slot % PV_RING_K);
}
