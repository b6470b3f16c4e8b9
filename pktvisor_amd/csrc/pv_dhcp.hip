// SPDX-License-Identifier: MPL-2.0
// pv_dhcp.hip — the DHCP handler's device stage (gfx950). It runs only while the handler is
// attached (pv_set_dhcp), next to the Net / DNS passes and without touching them:
//
//   pv_dhcp_scan    one lane per record: is it a DHCP packet (a UDP packet, as parse_record sees
//                   one, on port 67 / 68, else 546 / 547)? Ethernet + IPv4 / IPv6 without
//                   extension headers are answered from the 80-byte header window the Net pass
//                   reads (five 16-B loads from the record's 4-aligned start), everything else by
//                   parse_record over HBM. Per 64-record tile: the wave's ballot as one 64-bit
//                   mask and its popcount, stored by one lane. No per-record stores, no atomics.
//   (host)          pv_exclusive_scan_u32 over the tile counts: each tile's rank base
//   pv_dhcp_decode  flagged records only: the shared decoder (pv_dhcp.h) writes one PvDhcpEvent
//                   at the record's rank (record order: the host replay depends on it); the
//                   hostname bytes of REQUESTs go to a byte arena claimed with one atomicAdd each.
//                   A round stores the events of ranks [base, base + cap).
#include <hip/hip_runtime.h>

#include "pv_layout.h"

#define PV_C __attribute__((address_space(4)))
#define PV_CREF(T) const PV_C T &
#define PV_FN __device__ __forceinline__
__device__ __forceinline__ uint32_t pv_clz64(uint64_t x) { return (uint32_t)__clzll((long long)x); }
__device__ __forceinline__ uint32_t pv_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
#include "pv_parse.h"
#define PV_DHCP_NO_MANAGER
#include "pv_dhcp.h"

namespace {

// HBM accessor (recs is padded by PV_RECS_PAD: two aligned dword loads give an unaligned u32)
struct DAcc {
    const PV_G uint8_t *R;
    PV_FN uint32_t u32(uint64_t off) const
    {
        const PV_G uint32_t *p = reinterpret_cast<const PV_G uint32_t *>(R + (off & ~3ull));
        return __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)(off & 3));
    }
    PV_FN uint32_t u32a(uint64_t off) const { return *reinterpret_cast<const PV_G uint32_t *>(R + off); }
    PV_FN uint32_t u8(uint64_t off) const { return R[off]; }
};

PV_FN uint32_t bswap16(uint32_t v) { return ((v & 0xff) << 8) | ((v >> 8) & 0xff); }

// The header-window answer for a linktype-1 record: 1 = DHCP, 0 = not, 2 = ask parse_record.
// w[j] = bytes [4j, 4j + 4) from the record's start (16-byte record header, then the frame), so
// the Ethernet type is w[7]'s low half and an IP header starts at byte 30. Each branch restates
// parse_record's general walk for that frame shape and gives up on anything else.
PV_FN uint32_t dhcp_fast(const uint32_t (&w)[19])
{
    const uint32_t caplen = w[2];
    if (caplen <= 14) return 0; // no L2 payload: no IP header is located
    const uint32_t et = bswap16(w[7] & 0xffff);
    uint32_t len = caplen - 14;
    if (et == 0x0800) {
        const uint32_t b0 = (w[7] >> 16) & 0xff, ihl = b0 & 15;
        if (len < 20 || (b0 >> 4) != 4 || ihl < 5) return 0;
        if (ihl > 10) return 2; // ports beyond the window
        const uint32_t total = bswap16(w[8] & 0xffff);
        if (total < len && total != 0) len = total;
        const uint32_t hl = ihl * 4;
        if (len <= hl) return 0;
        if (bswap16(w[9] & 0xffff) & 0x3fff) return 0; // a fragment (first or later) has no L4 layer
        const uint32_t proto = w[9] >> 24;
        if (proto == 4 || proto == 41) return 2; // a tunnel
        if (proto != 17 || len - hl < 8) return 0;
        // the UDP header's first word: byte 30 + hl = 4 * (12 + (ihl - 5)) + 2
        uint32_t pw = 0;
#pragma unroll
        for (uint32_t k = 0; k < 6; k++)
            if (ihl == 5 + k) pw = __builtin_amdgcn_alignbyte(w[13 + k], w[12 + k], 2);
        return dhcp_family_of_ports(pw) ? 1 : 0;
    }
    if (et == 0x86DD) {
        if (len < 40) return 0;
        const uint32_t next = w[9] & 0xff;
        if (next == 0 || next == 60 || next == 43 || next == 44 || next == 51 || next == 4 || next == 41) return 2;
        if (next != 17) return 0;
        const uint32_t total = bswap16(w[8] >> 16) + 40;
        if (total < len) len = total;
        if (len <= 40 || len - 40 < 8) return 0;
        return dhcp_family_of_ports(__builtin_amdgcn_alignbyte(w[18], w[17], 2)) ? 1 : 0; // byte 70
    }
    if (et == 0x8100 || et == 0x88A8) return 2;
    return 0; // no IP header behind this type
}

PV_FN ParseCfg dhcp_cfg(uint32_t linktype, uint32_t ts_nano)
{
    ParseCfg C;
    C.linktype = linktype;
    C.ts_nano = ts_nano;
    C.n4 = 0; // direction is not needed: no subnet is matched
    C.a0 = C.a1 = 0;
    C.m0 = C.m1 = 0xffffffffu;
    return C;
}

} // namespace

// P: a zeroed PvParams (parse_record reads its host subnets only; none here).
// mask / cnt: one entry per 64-record tile, ntiles = ceil(n / 64).
extern "C" __global__ void __launch_bounds__(256) pv_dhcp_scan(const uint8_t *__restrict__ recs_, const uint32_t *__restrict__ offs_,
                                                                uint32_t n, uint32_t linktype, uint32_t ts_nano,
                                                                const PvParams *__restrict__ Pp, unsigned long long *__restrict__ mask,
                                                                uint32_t *__restrict__ cnt)
{
    PV_CREF(PvParams) P = *(const PV_C PvParams *)Pp;
    const PV_G uint8_t *const recs = (const PV_G uint8_t *)recs_;
    const PV_G uint32_t *const offs = (const PV_G uint32_t *)offs_;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t ntiles = (n + 63) / 64;
    const uint32_t wpb = blockDim.x >> 6;
    const ParseCfg C = dhcp_cfg(linktype, ts_nano);
    for (uint32_t t = blockIdx.x * wpb + (threadIdx.x >> 6); t < ntiles; t += gridDim.x * wpb) {
        const uint32_t i = t * 64 + lane;
        const bool active = i < n;
        const uint32_t off = offs[active ? i : n - 1];
        uint32_t verdict = 2;
        if (linktype == 1) {
            const PV_G uint4 *p = reinterpret_cast<const PV_G uint4 *>(recs + (off & ~3u));
            uint32_t x[20];
#pragma unroll
            for (int j = 0; j < 5; j++) {
                const uint4 v = p[j];
                x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
            }
            uint32_t w[19];
#pragma unroll
            for (int j = 0; j < 19; j++) w[j] = __builtin_amdgcn_alignbyte(x[j + 1], x[j], off & 3);
            verdict = dhcp_fast(w);
        }
        if (active && verdict == 2) {
            const DAcc R{recs};
            Parsed o;
            parse_record(R, C, P, (uint64_t)off, o);
            verdict = dhcp_family(R, o) ? 1 : 0;
        }
        const unsigned long long m = __ballot(active && verdict == 1);
        if (lane == 0) {
            mask[t] = m;
            cnt[t] = (uint32_t)__popcll(m);
        }
    }
}

// Events of ranks [base, base + cap) into ev[rank - base]; arena_top counts the arena's bytes.
extern "C" __global__ void __launch_bounds__(256) pv_dhcp_decode(const uint8_t *__restrict__ recs_, const uint32_t *__restrict__ offs_,
                                                                  uint32_t n, uint32_t linktype, uint32_t ts_nano,
                                                                  const PvParams *__restrict__ Pp,
                                                                  const unsigned long long *__restrict__ mask,
                                                                  const uint32_t *__restrict__ rank, uint32_t base, uint32_t cap,
                                                                  PvDhcpEvent *__restrict__ ev, uint8_t *__restrict__ arena,
                                                                  uint32_t arena_cap, uint32_t *__restrict__ arena_top)
{
    PV_CREF(PvParams) P = *(const PV_C PvParams *)Pp;
    const PV_G uint8_t *const recs = (const PV_G uint8_t *)recs_;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t t = i >> 6, lane = i & 63;
    const unsigned long long m = mask[t];
    if (!((m >> lane) & 1)) return;
    const uint32_t r = rank[t] + (uint32_t)__popcll(m & ((1ull << lane) - 1));
    if (r < base || r - base >= cap) return;
    const uint32_t off = offs_[i];
    const DAcc R{recs};
    const ParseCfg C = dhcp_cfg(linktype, ts_nano);
    Parsed o;
    parse_record(R, C, P, (uint64_t)off, o);
    const uint32_t fam = dhcp_family(R, o);
    PvDhcpEvent e;
    uint64_t host_at = 0;
    // (the scan flagged this record with the same parse, so fam is 4 or 6)
    dhcp_decode(R, linktype, o, fam ? fam : 4u, i, e, host_at);
    if (e.family == 4 && e.mtype == 3 && e.host_len) {
        // a REQUEST's hostname: the only bytes the manager keeps
        const uint32_t at = atomicAdd(arena_top, (uint32_t)e.host_len);
        if (at + e.host_len <= arena_cap) {
            e.host_off = at;
            for (uint32_t k = 0; k < e.host_len; k++) arena[at + k] = recs[host_at + k];
        } else e.host_len = 0; // cannot happen: the arena holds cap * 255 bytes
    }
    ev[r - base] = e;
}
