// SPDX-License-Identifier: MPL-2.0
// pv_flow.hip — the flow handler's device stage (gfx950). It runs only while the handler is
// attached (pv_set_flow), next to the Net / DNS / DHCP / BGP passes and without touching them:
//
//   pv_flow_scan    one lane per record: is it a NetFlow v1 / v5 / v7 datagram (a UDP packet, as
//                   parse_record sees one, to a configured port, whose payload passes flow_check),
//                   and how many flow records does it carry? Ethernet + IPv4 (IHL 5..10) / IPv6
//                   without extension headers are answered from the header window the Net pass
//                   reads (five 16-B loads from the record's 4-aligned start): the UDP test and the
//                   port test always, the NetFlow common header too where it lies inside the
//                   window's 76 usable bytes (IPv4 with IHL 5..8). For IHL 9 / 10 and IPv6 the
//                   common header starts at record byte 74 / 78, behind the window: those lanes,
//                   already known to be UDP on a configured port, load that one word. Everything
//                   else goes through parse_record over HBM. Per 64-record tile one lane stores the
//                   ballot mask of datagrams, their number, the tile's sum of flow-record counts (a
//                   wave reduction) and the two counts of refused payloads. No per-record stores,
//                   no atomics.
//   (host)          one pv_exclusive_scan_u32 over the four per-tile arrays laid end to end (and
//                   a closing 0): each tile's rank bases, each array's total
//   pv_flow_decode  one wave per tile, flagged records only: a PvFlowPacket at the datagram's rank
//                   and its PvFlowRecords at consecutive ranks from its first record's rank (the
//                   tile's base plus an in-wave exclusive prefix over the lanes' counts, by
//                   __shfl_up). Both lists are in record order: the host replay depends on it.
//                   A round stores the datagrams whose first record's rank is in [fbase, fbase +
//                   cap), each of them whole: the record buffer holds cap + 29 records. The one
//                   datagram that holds the round's last record stores where the next round begins.
#include <hip/hip_runtime.h>

#include "pv_layout.h"

#define PV_C __attribute__((address_space(4)))
#define PV_CREF(T) const PV_C T &
#define PV_FN __device__ __forceinline__
__device__ __forceinline__ uint32_t pv_clz64(uint64_t x) { return (uint32_t)__clzll((long long)x); }
__device__ __forceinline__ uint32_t pv_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
#include "pv_parse.h"
#define PV_FLOW_NO_MANAGER
#include "pv_flow.h"

namespace {

// HBM accessor (recs is padded by PV_RECS_PAD: two aligned dword loads give an unaligned u32)
struct FAcc {
    const PV_G uint8_t *R;
    PV_FN uint32_t u32(uint64_t off) const
    {
        const PV_G uint32_t *p = reinterpret_cast<const PV_G uint32_t *>(R + (off & ~3ull));
        return __builtin_amdgcn_alignbyte(p[1], p[0], (uint32_t)(off & 3));
    }
    PV_FN uint32_t u32a(uint64_t off) const { return *reinterpret_cast<const PV_G uint32_t *>(R + off); }
    PV_FN uint32_t u8(uint64_t off) const { return R[off]; }
};

// The header-window answer for a linktype-1 record: 0 = not a UDP packet to a configured port,
// 2 = ask parse_record, 1 = a candidate whose UDP header starts at record byte `udp` and whose
// IP-length-trimmed L4 layer has l4len bytes (inside the captured bytes: len <= caplen - 14), with
// the payload's first word in hw when have_hw. w[j] = bytes [4j, 4j + 4) from the record's start
// (16-byte record header, then the frame). Each branch restates parse_record's general walk for
// that frame shape, as dhcp_fast does, and gives up on anything else.
PV_FN uint32_t flow_fast(const uint32_t (&w)[19], const PvFlowPorts &L, uint32_t &udp, uint32_t &l4len, uint32_t &hw, bool &have_hw)
{
    have_hw = false;
    const uint32_t caplen = w[2];
    if (caplen <= 14) return 0;
    const uint32_t et = flow_bswap16(w[7] & 0xffff);
    uint32_t len = caplen - 14;
    if (et == 0x0800) {
        const uint32_t b0 = (w[7] >> 16) & 0xff, ihl = b0 & 15;
        if (len < 20 || (b0 >> 4) != 4 || ihl < 5) return 0;
        if (ihl > 10) return 2;
        const uint32_t total = flow_bswap16(w[8] & 0xffff);
        if (total < len && total != 0) len = total;
        const uint32_t hl = ihl * 4;
        if (len <= hl) return 0;
        if (flow_bswap16(w[9] & 0xffff) & 0x3fff) return 0;
        const uint32_t proto = w[9] >> 24;
        if (proto == 4 || proto == 41) return 2;
        if (proto != 17 || len - hl < 8) return 0;
        // the UDP header's first word at byte 30 + hl = 4 * (12 + (ihl - 5)) + 2, the payload's two words on
        uint32_t pw = 0;
#pragma unroll
        for (uint32_t k = 0; k < 6; k++)
            if (ihl == 5 + k) pw = __builtin_amdgcn_alignbyte(w[13 + k], w[12 + k], 2);
        if (!flow_port_ok(L, pw)) return 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (ihl == 5 + k) { hw = __builtin_amdgcn_alignbyte(w[15 + k], w[14 + k], 2); have_hw = true; }
        udp = 30 + hl;
        l4len = len - hl;
        return 1;
    }
    if (et == 0x86DD) {
        if (len < 40) return 0;
        const uint32_t next = w[9] & 0xff;
        if (next == 0 || next == 60 || next == 43 || next == 44 || next == 51 || next == 4 || next == 41) return 2;
        if (next != 17) return 0;
        const uint32_t total = flow_bswap16(w[8] >> 16) + 40;
        if (total < len) len = total;
        if (len <= 40 || len - 40 < 8) return 0;
        if (!flow_port_ok(L, __builtin_amdgcn_alignbyte(w[18], w[17], 2))) return 0; // byte 70
        udp = 70;
        l4len = len - 40;
        return 1;
    }
    if (et == 0x8100 || et == 0x88A8) return 2;
    return 0;
}

PV_FN ParseCfg flow_cfg(uint32_t linktype, uint32_t ts_nano)
{
    ParseCfg C;
    C.linktype = linktype;
    C.ts_nano = ts_nano;
    C.n4 = 0; // direction is not needed: no subnet is matched
    C.a0 = C.a1 = 0;
    C.m0 = C.m1 = 0xffffffffu;
    return C;
}

PV_FN uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

} // namespace

// P: a zeroed PvParams (parse_record reads its host subnets only; none here).
// mask: one entry per 64-record tile, ntiles = ceil(n / 64). tile: 4 * ntiles + 1 entries, four
// arrays laid end to end (datagrams, flow records, refused payloads, refused payloads of version 9
// or 10) and a closing 0, so that one exclusive scan gives every rank base and every total.
extern "C" __global__ void __launch_bounds__(256) pv_flow_scan(const uint8_t *__restrict__ recs_, const uint32_t *__restrict__ offs_,
                                                                uint32_t n, uint32_t linktype, uint32_t ts_nano,
                                                                const PvParams *__restrict__ Pp, PvFlowPorts L,
                                                                unsigned long long *__restrict__ mask, uint32_t *__restrict__ tile)
{
    PV_CREF(PvParams) P = *(const PV_C PvParams *)Pp;
    const PV_G uint8_t *const recs = (const PV_G uint8_t *)recs_;
    const PV_G uint32_t *const offs = (const PV_G uint32_t *)offs_;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t ntiles = (n + 63) / 64;
    const uint32_t wpb = blockDim.x >> 6;
    const ParseCfg C = flow_cfg(linktype, ts_nano);
    const FAcc R{recs};
    if (blockIdx.x == 0 && threadIdx.x == 0) tile[4 * ntiles] = 0;
    for (uint32_t t = blockIdx.x * wpb + (threadIdx.x >> 6); t < ntiles; t += gridDim.x * wpb) {
        const uint32_t i = t * 64 + lane;
        const bool active = i < n;
        const uint32_t off = offs[active ? i : n - 1];
        uint32_t verdict = 2, count = 0, version = 0;
        bool cand = false;
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
            uint32_t udp = 0, l4len = 0, hw = 0;
            bool have_hw = false;
            verdict = flow_fast(w, L, udp, l4len, hw, have_hw);
            if (active && verdict == 1) {
                cand = true;
                const uint32_t plen = l4len - 8; // (not clipped: the L4 layer lies inside the captured bytes)
                if (plen >= 4) {
                    if (!have_hw) hw = R.u32((uint64_t)off + udp + 8);
                    count = flow_check(hw, plen, version);
                }
            }
        }
        if (active && verdict == 2) {
            Parsed o;
            parse_record(R, C, P, (uint64_t)off, o);
            count = flow_classify(R, o, L, cand, version);
        }
        const bool bad = active && cand && count == 0;
        const unsigned long long m = __ballot(active && count != 0);
        const unsigned long long mb = __ballot(bad), m9 = __ballot(bad && (version == 9 || version == 10));
        const uint32_t sum = wave_sum(active ? count : 0u);
        if (lane == 0) {
            mask[t] = m;
            tile[t] = (uint32_t)__popcll(m);
            tile[ntiles + t] = sum;
            tile[2 * ntiles + t] = (uint32_t)__popcll(mb);
            tile[3 * ntiles + t] = (uint32_t)__popcll(m9);
        }
    }
}

// tile / scan: pv_flow_scan's per-tile array and its exclusive scan. The datagrams whose first
// record's rank f has fbase <= f < fbase + cap: the packet of datagram rank r to pk[r - dbase]
// (dbase: the rank of the round's first datagram; pk holds pcap entries), its records to
// fr[f - fbase + j] (fr holds cap + PV_FLOW_SLACK). nrec: the
// batch's number of flow records. next[0] / next[1]: the dbase / fbase of the round after this one.
extern "C" __global__ void __launch_bounds__(256) pv_flow_decode(const uint8_t *__restrict__ recs_, const uint32_t *__restrict__ offs_,
                                                                  uint32_t n, uint32_t linktype, uint32_t ts_nano,
                                                                  const PvParams *__restrict__ Pp, PvFlowPorts L,
                                                                  const unsigned long long *__restrict__ mask,
                                                                  const uint32_t *__restrict__ tile, const uint32_t *__restrict__ scan,
                                                                  uint32_t dbase, uint32_t fbase, uint32_t cap, uint32_t pcap, uint32_t nrec,
                                                                  PvFlowPacket *__restrict__ pk, PvFlowRecord *__restrict__ fr,
                                                                  uint32_t *__restrict__ next)
{
    PV_CREF(PvParams) P = *(const PV_C PvParams *)Pp;
    const PV_G uint8_t *const recs = (const PV_G uint8_t *)recs_;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t ntiles = (n + 63) / 64;
    const uint32_t wpb = blockDim.x >> 6;
    const ParseCfg C = flow_cfg(linktype, ts_nano);
    const FAcc R{recs};
    // (64-bit: fbase + cap may pass 2^32)
    const uint64_t round_end = (uint64_t)fbase + cap, last = round_end < nrec ? round_end : (uint64_t)nrec;
    for (uint32_t t = blockIdx.x * wpb + (threadIdx.x >> 6); t < ntiles; t += gridDim.x * wpb) {
        const unsigned long long m = mask[t];
        if (!m) continue;
        const uint32_t tbase = scan[ntiles + t] - scan[ntiles], tcount = tile[ntiles + t];
        if (tbase >= round_end || tbase + tcount <= fbase) continue;
        const uint32_t i = t * 64 + lane;
        const bool flagged = (m >> lane) & 1;
        uint32_t count = 0, version = 0;
        Parsed o;
        if (flagged) {
            bool cand;
            parse_record(R, C, P, (uint64_t)offs_[i], o);
            count = flow_classify(R, o, L, cand, version); // (the scan flagged this record with the same checks)
        }
        // in-wave inclusive prefix of the lanes' counts
        uint32_t incl = count;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += up;
        }
        const uint32_t first = tbase + incl - count;
        if (!flagged || count == 0 || first < fbase || first >= round_end) continue;
        const uint32_t r = scan[t] + (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (r < dbase || r - dbase >= pcap) continue; // (cannot happen: r - dbase <= first - fbase, and pcap covers it)
        PvFlowPacket p;
        flow_decode_packet(R, o, i, version, count, first, p);
        pk[r - dbase] = p;
        const uint64_t pay = o.l4off + 8;
        for (uint32_t j = 0; j < count; j++) {
            PvFlowRecord f;
            flow_decode_record(R, pay + flow_record_at(version, j), f);
            fr[first - fbase + j] = f;
        }
        if ((uint64_t)first + count >= last) {
            next[0] = r + 1;
            next[1] = first + count;
        }
    }
}
