// SPDX-License-Identifier: MPL-2.0
// pv_bgp.hip — the BGP handler's device stage (gfx950). It runs only while the handler is
// attached (pv_set_bgp), next to the Net / DNS / DHCP passes and without touching them:
//
//   pv_bgp_scan        one lane per record: is it a TCP record, and is it a BGP segment (pv_bgp.h
//                      bgp_is_segment: port 179 on either side, a payload or SYN / FIN / RST)?
//                      Ethernet + IPv4 / IPv6 without extension headers are answered from the
//                      80-byte header window the Net pass reads (five 16-B loads from the record's
//                      4-aligned start) as long as no port is 179; port-179 records and everything
//                      else go through parse_record over HBM. Per 64-record tile one lane stores
//                      the wave's ballot as a 64-bit mask, its popcount, and the greatest seconds
//                      value of the tile's TCP records (any port, 0 = none; a DPP reduction). No
//                      per-record stores, no atomics.
//   (host)             pv_exclusive_scan_u32 over the tile counts: each tile's rank base;
//   pv_bgp_prefix_max  rocPRIM inclusive max-scan over the tiles' TCP seconds
//   pv_bgp_decode      one wave per tile, tiles without a segment of the round leave at once: the
//                      lanes parse their records, a shuffle prefix-max gives every lane the greatest
//                      TCP second before it (exact inside the tile; the tiles before it come from
//                      the prefix), flagged lanes write their PvBgpSeg at their rank (record order:
//                      the host replay depends on it) and copy their payload, in whole dwords, into
//                      a byte arena claimed with one atomicAdd each. A round stores ranks
//                      [base, base + cap).
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "pv_layout.h"

#define PV_C __attribute__((address_space(4)))
#define PV_CREF(T) const PV_C T &
#define PV_FN __device__ __forceinline__
__device__ __forceinline__ uint32_t pv_clz64(uint64_t x) { return (uint32_t)__clzll((long long)x); }
__device__ __forceinline__ uint32_t pv_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
#include "pv_parse.h"
#define PV_BGP_NO_MANAGER
#include "pv_bgp.h"

namespace {

// HBM accessor (recs is padded by PV_RECS_PAD: two aligned dword loads give an unaligned u32)
struct BAcc {
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

// The header-window answer for a linktype-1 record: 0 = no TCP record, 1 = a TCP record without
// port 179 (no segment), 2 = ask parse_record (port 179, or a frame shape beyond the window).
// w[j] = bytes [4j, 4j + 4) from the record's start (16-byte record header, then the frame), so
// the Ethernet type is w[7]'s low half and an IP header starts at byte 30. Each branch restates
// parse_record's general walk for that frame shape and gives up on anything else.
PV_FN uint32_t bgp_fast(const uint32_t (&w)[19])
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
        if (proto != 6 || len - hl < 20) return 0;
        // the TCP header's first word: byte 30 + hl = 4 * (12 + (ihl - 5)) + 2
        uint32_t pw = 0;
#pragma unroll
        for (uint32_t k = 0; k < 6; k++)
            if (ihl == 5 + k) pw = __builtin_amdgcn_alignbyte(w[13 + k], w[12 + k], 2);
        return bgp_ports(pw) ? 2 : 1;
    }
    if (et == 0x86DD) {
        if (len < 40) return 0;
        const uint32_t next = w[9] & 0xff;
        if (next == 0 || next == 60 || next == 43 || next == 44 || next == 51 || next == 4 || next == 41) return 2;
        if (next != 6) return 0;
        const uint32_t total = bswap16(w[8] >> 16) + 40;
        if (total < len) len = total;
        if (len <= 40 || len - 40 < 20) return 0;
        return bgp_ports(__builtin_amdgcn_alignbyte(w[18], w[17], 2)) ? 2 : 1; // byte 70
    }
    if (et == 0x8100 || et == 0x88A8) return 2;
    return 0; // no IP header behind this type
}

// a lane's operand for the reduction below: the value of the lane CTRL names (row_shr:n), 0 where none
template <int CTRL>
PV_FN uint32_t dpp_umax_src(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false); }

PV_FN ParseCfg bgp_cfg(uint32_t linktype, uint32_t ts_nano)
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
// mask / cnt / tsec: one entry per 64-record tile, ntiles = ceil(n / 64).
extern "C" __global__ void __launch_bounds__(256) pv_bgp_scan(const uint8_t *__restrict__ recs_, const uint32_t *__restrict__ offs_,
                                                               uint32_t n, uint32_t linktype, uint32_t ts_nano,
                                                               const PvParams *__restrict__ Pp, unsigned long long *__restrict__ mask,
                                                               uint32_t *__restrict__ cnt, uint32_t *__restrict__ tsec)
{
    PV_CREF(PvParams) P = *(const PV_C PvParams *)Pp;
    const PV_G uint8_t *const recs = (const PV_G uint8_t *)recs_;
    const PV_G uint32_t *const offs = (const PV_G uint32_t *)offs_;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t ntiles = (n + 63) / 64;
    const uint32_t wpb = blockDim.x >> 6;
    const ParseCfg C = bgp_cfg(linktype, ts_nano);
    for (uint32_t t = blockIdx.x * wpb + (threadIdx.x >> 6); t < ntiles; t += gridDim.x * wpb) {
        const uint32_t i = t * 64 + lane;
        const bool active = i < n;
        const uint32_t off = offs[active ? i : n - 1];
        uint32_t verdict = 2, ts = 0; // ts: the record's second when it is a TCP record
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
            verdict = bgp_fast(w);
            ts = active && verdict == 1 ? w[0] : 0u;
        }
        bool seg = false;
        if (active && verdict == 2) {
            const BAcc R{recs};
            Parsed o;
            parse_record(R, C, P, (uint64_t)off, o);
            ts = bgp_is_tcp(o) ? (uint32_t)o.sec : 0u;
            seg = bgp_is_segment(R, o);
        }
        const unsigned long long m = __ballot(seg);
        // the tile's greatest TCP second, in lane 63: a DPP reduction (row shifts inside the four
        // 16-lane rows, then lane 15 / 31 broadcast into the rows behind; 0 is the identity)
        ts = max(ts, dpp_umax_src<0x111>(ts));
        ts = max(ts, dpp_umax_src<0x112>(ts));
        ts = max(ts, dpp_umax_src<0x114>(ts));
        ts = max(ts, dpp_umax_src<0x118>(ts));
        ts = max(ts, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ts, 0x142, 0xa, 0xf, false));
        ts = max(ts, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)ts, 0x143, 0xc, 0xf, false));
        if (lane == 63) {
            mask[t] = m;
            cnt[t] = (uint32_t)__popcll(m);
            tsec[t] = ts;
        }
    }
}

// Inclusive prefix maximum of n u32 (rocPRIM), tmp sized by a first call with tmp == nullptr.
extern "C" hipError_t pv_bgp_prefix_max(void *tmp, size_t *tmp_bytes, const uint32_t *in, uint32_t *out, size_t n, hipStream_t s)
{
    return rocprim::inclusive_scan(tmp, *tmp_bytes, in, out, n, rocprim::maximum<uint32_t>(), s);
}

// Segments of ranks [base, base + cap) into seg[rank - base]; tincl: the inclusive prefix maximum of
// the tiles' TCP seconds; arena_top counts the bytes the round's payloads ask for (the host reruns
// a round that asked for more than arena_cap over fewer ranks). Launched with one thread per
// record in blocks of 256: a wave is a tile.
extern "C" __global__ void __launch_bounds__(256) pv_bgp_decode(const uint8_t *__restrict__ recs_, const uint32_t *__restrict__ offs_,
                                                                 uint32_t n, uint32_t linktype, uint32_t ts_nano,
                                                                 const PvParams *__restrict__ Pp,
                                                                 const unsigned long long *__restrict__ mask,
                                                                 const uint32_t *__restrict__ rank, const uint32_t *__restrict__ tincl,
                                                                 uint32_t base, uint32_t cap, PvBgpSeg *__restrict__ seg,
                                                                 uint8_t *__restrict__ arena, uint32_t arena_cap,
                                                                 unsigned long long *__restrict__ arena_top)
{
    PV_CREF(PvParams) P = *(const PV_C PvParams *)Pp;
    const PV_G uint8_t *const recs = (const PV_G uint8_t *)recs_;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t t = i >> 6, lane = i & 63;
    if (t >= (n + 63) / 64) return; // (whole waves)
    const unsigned long long m = mask[t];
    const uint64_t r0 = rank[t];
    if (!m || r0 + (uint32_t)__popcll(m) <= base || r0 >= (uint64_t)base + cap) return; // no segment of this round in the tile
    const bool active = i < n;
    const BAcc R{recs};
    Parsed o;
    uint32_t v = 0;
    if (active) {
        parse_record(R, bgp_cfg(linktype, ts_nano), P, (uint64_t)offs_[i], o);
        if (bgp_is_tcp(o)) v = (uint32_t)o.sec;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= (uint32_t)d && u > v) v = u;
    }
    uint32_t before = (uint32_t)__shfl_up((int)v, 1, 64);
    if (lane == 0) before = 0;
    const uint32_t prev = t ? tincl[t - 1] : 0u;
    if (prev > before) before = prev;
    if (!active || !((m >> lane) & 1)) return;
    const uint32_t r = (uint32_t)r0 + (uint32_t)__popcll(m & ((1ull << lane) - 1));
    if (r < base || r - base >= cap) return;
    PvBgpSeg g;
    uint64_t pay_at = 0;
    if (!bgp_segment(R, o, g, pay_at)) {
        // (the scan flagged this record with the same test: not reached)
        g = PvBgpSeg{};
        g.sec = (uint32_t)o.sec;
    }
    g.rec = i;
    g.tcp_sec_before = before;
    g.off = 0;
    if (g.caplen) {
        // claimed and copied in whole dwords: the claim is rounded up to four bytes, so the last
        // store stays inside it, and the loads past the payload's end stay inside the blob's padding
        const uint32_t words = (g.caplen + 3) / 4;
        const unsigned long long at = atomicAdd(arena_top, (unsigned long long)words * 4);
        if (at + (unsigned long long)words * 4 <= arena_cap) {
            g.off = (uint32_t)at;
            uint32_t *dst = reinterpret_cast<uint32_t *>(arena + at);
            for (uint32_t k = 0; k < words; k++) dst[k] = R.u32(pay_at + 4ull * k);
        }
    }
    seg[r - base] = g;
}
