// SPDX-License-Identifier: MPL-2.0
// pv_dhcp.h — the DHCP handler (src/handlers/dhcp in the reference): the event the device
// stage produces, the packet decoder shared by the device kernels and the CPU test harness,
// and the host manager that replays the ordered event list.
//
// Split: finding and decoding DHCP packets looks at every record of a batch (pv_dhcp.hip);
// what is found is a handful of events whose semantics are strictly sequential (period
// shifts on the manager's own events, one jsf32 draw per event, a transaction map a later
// REQUEST overwrites), so the host manager (pv_dhcp.cpp) replays them in record order.
//
// The decoder part needs pv_parse.h included first (it is compiled only when PV_FN is
// defined, with the accessor interface documented there); the manager part is plain C++.
#pragma once
#include <stdint.h>

// One decoded DHCP / DHCPv6 packet, written at its rank among the batch's DHCP packets
// (record order). Multi-byte wire fields keep their wire byte order (a little-endian load
// of the network-order bytes).
struct PvDhcpEvent {
    uint32_t rec;       // record index in the batch
    uint32_t sec, nsec; // the record's stamp (nsec at the record's precision)
    uint32_t xid;       // BOOTP transaction id (v4)
    uint32_t yiaddr;    // "your" address (v4)
    uint32_t server_id; // option 54's first four bytes, 0 with fewer (v4)
    uint32_t host_off;  // hostname bytes: offset into the hostname arena (REQUEST only)
    uint16_t host_len;  // 0..255
    uint8_t family;     // 4 = DHCP (ports 67 / 68), 6 = DHCPv6 (ports 546 / 547)
    uint8_t mtype;      // message type (option 53 / byte 0), 0 when absent
    uint8_t flags;      // PV_DHCP_F_*
    uint8_t cmac[6];    // chaddr[0..6) when htype == 1 and hlen == 6, else zeros
    uint8_t emac[6];    // Ethernet source address (PV_DHCP_F_ETH)
    uint8_t pad[3];
    uint8_t v6src[16];  // source address of the first IPv6 header (PV_DHCP_F_V6SRC)
};
static_assert(sizeof(PvDhcpEvent) == 64 && sizeof(PvDhcpEvent) % 16 == 0, "PvDhcpEvent: 64 bytes");

#define PV_DHCP_F_SERVER 1u // v4: option 54 present; v6: option 2's header fits the payload
#define PV_DHCP_F_ETH 2u    // the packet has an Ethernet layer (link type 1)
#define PV_DHCP_F_V6SRC 4u  // the packet has an IPv6 header
#define PV_DHCP_F_HOST 8u   // option 12 present (its value may be empty)
#define PV_DHCP_HOST_MAX 255u

#ifdef PV_FN
// ------------------------------------------------------------------ decoder
// Which packets are DHCP (DhcpStreamHandler::process_udp_packet_cb, DhcpStreamHandler.cpp:21-39):
// a UDP packet as parse_record sees one (so fragments, VLAN tags, tunnels and IP-length
// trimming mean what they mean to the Net pass) with port 67 / 68 on either side (v4, on any
// L3), else 546 / 547 on either side (v6). 0 = not DHCP.
PV_FN uint32_t dhcp_family_of_ports(uint32_t pw) // pw: the UDP header's first word, little-endian load
{
    const uint32_t sp = ((pw & 0xff) << 8) | ((pw >> 8) & 0xff), dp = ((pw >> 8) & 0xff00) | (pw >> 24);
    if (sp == 67 || sp == 68 || dp == 67 || dp == 68) return 4;
    if (sp == 546 || sp == 547 || dp == 546 || dp == 547) return 6;
    return 0;
}
template <class A>
PV_FN uint32_t dhcp_family(const A &R, const Parsed &o)
{
    if (o.l4 != 17 || o.l4len < 8) return 0;
    return dhcp_family_of_ports(R.u32(o.l4off));
}

// Decode the message of a DHCP packet (fam from dhcp_family) into ev; the hostname's bytes stay
// in the record blob at [host_at, host_at + ev.host_len) for the caller to copy. Rules (restated
// from PcapPlusPlus's DhcpLayer / DhcpV6Layer / TLV reader, which is not vendored; parity on
// malformed input is unpinned):
//   payload  [l4off + 8, l4off + l4len) clipped to the captured bytes
//   v4       240-byte BOOTP header (magic not checked), then options type(1) len(1) value; PAD (0)
//            and END (255) are one byte; the walk does not stop at END, ends at the first record
//            that would pass the payload's end; the first record of a wanted type wins.
//            Message type = first byte of option 53 (0 if absent or empty); hostname = option 12;
//            server id = option 54 (0.0.0.0 with fewer than four bytes). A payload under 240
//            bytes is an event of type 0 and nothing else is taken from it (the reference reads
//            out of bounds there: our definition).
//   v6       byte 0 is the type (0 for an empty payload); options from byte 4 as type(2) len(2)
//            big endian; option 2 is present when its four-byte header fits the payload
template <class A>
PV_FN void dhcp_decode(const A &R, uint32_t linktype, const Parsed &o, uint32_t fam, uint32_t rec, PvDhcpEvent &ev,
                       uint64_t &host_at)
{
    ev.rec = rec;
    ev.sec = (uint32_t)o.sec;
    ev.nsec = (uint32_t)o.nsec;
    ev.xid = ev.yiaddr = ev.server_id = ev.host_off = 0;
    ev.host_len = 0;
    ev.family = (uint8_t)fam;
    ev.mtype = 0;
    ev.flags = 0;
    for (int k = 0; k < 6; k++) ev.cmac[k] = ev.emac[k] = 0;
    for (int k = 0; k < 3; k++) ev.pad[k] = 0;
    for (int k = 0; k < 16; k++) ev.v6src[k] = 0;
    host_at = 0;
    if (linktype == 1) {
        ev.flags |= PV_DHCP_F_ETH;
        for (uint32_t k = 0; k < 6; k++) ev.emac[k] = (uint8_t)R.u8(o.frame + 6 + k);
    }
    if (o.has6) {
        ev.flags |= PV_DHCP_F_V6SRC;
        for (uint32_t k = 0; k < 16; k++) ev.v6src[k] = (uint8_t)R.u8(o.v6 + 8 + k);
    }
    const uint64_t pay = o.l4off + 8, cap_end = o.frame + o.caplen;
    uint32_t plen = o.l4len - 8;
    const uint64_t avail = cap_end > pay ? cap_end - pay : 0;
    if (plen > avail) plen = (uint32_t)avail;
    if (fam == 4) {
        if (plen < 240) return;
        ev.xid = R.u32(pay + 4);
        ev.yiaddr = R.u32(pay + 16);
        if (R.u8(pay + 1) == 1 && R.u8(pay + 2) == 6)
            for (uint32_t k = 0; k < 6; k++) ev.cmac[k] = (uint8_t)R.u8(pay + 28 + k);
        bool have53 = false, have12 = false, have54 = false;
        uint32_t pos = 240;
        while (pos < plen) {
            const uint32_t t = R.u8(pay + pos);
            if (t == 0 || t == 255) { pos += 1; continue; }
            if (pos + 2 > plen) break;
            const uint32_t l = R.u8(pay + pos + 1);
            if (pos + 2 + l > plen) break;
            if (t == 53 && !have53) {
                have53 = true;
                ev.mtype = l ? (uint8_t)R.u8(pay + pos + 2) : 0;
            } else if (t == 12 && !have12) {
                have12 = true;
                ev.flags |= PV_DHCP_F_HOST;
                ev.host_len = (uint16_t)l;
                host_at = pay + pos + 2;
            } else if (t == 54 && !have54) {
                have54 = true;
                ev.flags |= PV_DHCP_F_SERVER;
                ev.server_id = l >= 4 ? R.u32(pay + pos + 2) : 0;
            }
            pos += 2 + l;
        }
    } else {
        if (plen == 0) return;
        ev.mtype = (uint8_t)R.u8(pay);
        uint32_t pos = 4;
        while (pos + 4 <= plen) {
            const uint32_t t = (R.u8(pay + pos) << 8) | R.u8(pay + pos + 1);
            const uint32_t l = (R.u8(pay + pos + 2) << 8) | R.u8(pay + pos + 3);
            if (t == 2) { ev.flags |= PV_DHCP_F_SERVER; break; }
            pos += 4 + l;
        }
    }
}
#endif // PV_FN

#if defined(__cplusplus) && !defined(PV_DHCP_NO_MANAGER)
// ------------------------------------------------------------------ host manager
#include <deque>
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace pvdhcp {

enum { C_EVENTS, C_DEEP, C_DISCOVER, C_OFFER, C_REQUEST, C_ACK, C_SOLICIT, C_ADVERTISE, C_REQUEST_V6, C_REPLY, C_TOTAL,
       C_FILTERED, C_N };

// DhcpMetricsBucket (DhcpStreamHandler.h:41-118): the base event counts, the ten counters and two
// exact string-to-count maps behind top_clients / top_servers
struct Bucket {
    int64_t start_sec = 0, start_nsec = 0, end_sec = 0, end_nsec = 0;
    bool read_only = false;
    uint64_t period_length = 0;
    uint64_t c[C_N] = {};
    std::map<std::string, uint64_t> clients, servers;
};

// jsf32, the managers' deep-sampling generator (3rd/rng/jsf.h; the same generator as pv_host.h's
// Jsf32, restated so that this file needs no HIP header)
struct Jsf32 {
    uint32_t a = 0xf1ea5eedu, b = 1, c = 1, d = 1;
    Jsf32() { for (int i = 0; i < 20; i++) next(); }
    static uint32_t rot(uint32_t x, uint32_t k) { return (x << k) | (x >> (32 - k)); }
    uint32_t next()
    {
        const uint32_t e = a - rot(b, 27);
        a = b ^ rot(c, 17);
        b = c + d;
        c = d + e;
        d = e + a;
        return d;
    }
};

// DhcpMetricsManager over the event list (DhcpStreamHandler.cpp:231-346, .h:120-146) with its own
// window (AbstractMetricsManager::new_event / _period_shift, src/AbstractMetricsManager.h:276-333)
// and request/ack TransactionManager (libs/visor_transaction/TransactionManager.h:51-106).
class Manager {
  public:
    Manager(uint32_t num_periods, uint32_t deep_sample_rate, uint32_t xact_ttl_ms);
    // a fresh handler: buckets, transactions, generator
    void reset();
    bool started() const { return started_; }
    // start_tstamp_signal (first call after a reset only), end_tstamp_signal, heartbeat_signal
    void set_start(int64_t sec, int64_t nsec);
    void set_end(int64_t sec, int64_t nsec);
    void check_period_shift(int64_t sec, int64_t nsec);
    // n events in record order; hostname bytes at arena + host_off
    void replay(const PvDhcpEvent *ev, size_t n, const uint8_t *arena, size_t arena_bytes);
    // bucket `period`, or the fold of the `period` newest (merged); false with the reference's
    // PeriodException text in err
    bool window(uint32_t period, bool merged, Bucket &out, std::string &err) const;
    size_t periods() const { return buckets_.size(); }
    size_t open_transactions() const { return xact_.size(); }
    // the "dhcp" object of window_json: {"period":{...},"wire_packets":{...},"top_clients":[...],...}
    static std::string json(const Bucket &b, size_t topn_count, uint32_t topn_percentile_threshold);
    // TopN::to_json's selection (src/Metrics.h:510-521,577-590), ties by name as pv_render.cpp orders them
    static std::vector<std::pair<std::string, uint64_t>> top(const std::map<std::string, uint64_t> &m, size_t topn_count,
                                                              uint32_t pct);

  private:
    struct Xact {
        int64_t sec, nsec;
        std::string hostname, mac;
    };
    void new_event(int64_t sec, int64_t nsec);
    void shift(int64_t sec, int64_t nsec);
    uint32_t num_periods_, rate_, ttl_s_ = 0, ttl_ms_ = 0;
    std::deque<Bucket> buckets_; // front = live
    int64_t next_shift_sec_ = 0;
    bool started_ = false, deep_now_ = true;
    Jsf32 rng_;
    std::unordered_map<uint32_t, Xact> xact_;
};

} // namespace pvdhcp
#endif
