// SPDX-License-Identifier: MPL-2.0
// pv_bgp.h — the BGP handler (src/handlers/bgp in the reference): the TCP segment the device
// stage extracts, the extraction rule shared by the device kernels and the CPU test harness,
// and the host manager that reassembles the segments and counts what TcpReassembly delivers.
//
// Split (as the DHCP handler's, pv_dhcp.h): finding the TCP/179 segments looks at every record
// of a batch (pv_bgp.hip); what is found is a handful of segments whose semantics are strictly
// sequential (per-connection reassembly, an LRU list of connections with a 30 s time-out, period
// shifts and jsf32 draws on the manager's own events), so the host manager (pv_bgp.cpp) replays
// them in record order.
//
// The extraction part needs pv_parse.h included first (it is compiled only when PV_FN is
// defined, with the accessor interface documented there); the manager part is plain C++.
#pragma once
#include <stdint.h>

// One TCP segment of a connection with port 179 on either side, written at its rank among the
// batch's segments (record order).
struct PvBgpSeg {
    uint32_t rec;            // record index in the batch
    uint32_t sec, nsec;      // the record's stamp (nsec at the record's precision)
    uint32_t tcp_sec_before; // greatest seconds value of any TCP record earlier in the batch, 0 = none
    uint32_t fkey;           // hash5Tuple flow key (pv_parse.h flowkey)
    uint32_t seq;            // sequence number, host order
    uint32_t plen;           // payload length: [l4off + hl, l4off + l4len)
    uint32_t caplen;         // ... clipped to the captured bytes: the bytes in the arena
    uint32_t off;            // payload bytes: offset into the round's byte arena
    uint16_t sport, dport;   // host order
    uint8_t flags;           // PV_BGP_F_*
    uint8_t pad[7];
    uint8_t src[16];         // source address of the packet's first IP layer (4 bytes and zeros for IPv4)
};
static_assert(sizeof(PvBgpSeg) == 64 && sizeof(PvBgpSeg) % 16 == 0, "PvBgpSeg: 64 bytes");

#define PV_BGP_F_FIN 1u // (TCP flag bits 0..2 as on the wire)
#define PV_BGP_F_SYN 2u
#define PV_BGP_F_RST 4u
#define PV_BGP_F_V6 8u        // src is an IPv6 address
#define PV_BGP_PORT 179u
#define PV_BGP_PAY_MAX 65535u // a segment's payload (an IPv4 total length of 0 on a longer capture is clipped here)
#define PV_BGP_ARENA_MIN 65536u

#ifdef PV_FN
// ------------------------------------------------------------------ extraction
// pw: the TCP header's first word, little-endian load of the network-order ports
PV_FN bool bgp_ports(uint32_t pw)
{
    const uint32_t sp = ((pw & 0xff) << 8) | ((pw >> 8) & 0xff), dp = ((pw >> 8) & 0xff00) | (pw >> 24);
    return sp == PV_BGP_PORT || dp == PV_BGP_PORT;
}
// a TCP record: what drives the reassembly's time-outs, on any port (PcapInputStream's TCP branch)
PV_FN bool bgp_is_tcp(const Parsed &o) { return o.l4 == 6; }

// Is the record a BGP segment? A TCP packet as parse_record sees one (so fragments, VLAN tags,
// tunnels and IP-length trimming mean what they mean to the Net pass) whose header is a TcpLayer
// (20 <= hl <= l4len), with port 179 on either side, that TcpReassembly does not drop at once (a
// payload, or one of SYN / FIN / RST).
template <class A>
PV_FN bool bgp_is_segment(const A &R, const Parsed &o, uint32_t &pw, uint32_t &hl, uint32_t &fl, uint32_t &plen)
{
    if (!bgp_is_tcp(o)) return false;
    pw = R.u32(o.l4off);
    if (!bgp_ports(pw)) return false;
    const uint32_t w3 = R.u32(o.l4off + 12); // data offset (byte 12), flags (byte 13)
    hl = ((w3 >> 4) & 0xf) * 4;
    if (hl < 20 || hl > o.l4len) return false;
    fl = (w3 >> 8) & 7;
    plen = o.l4len - hl;
    if (plen > PV_BGP_PAY_MAX) plen = PV_BGP_PAY_MAX;
    return plen || fl;
}
template <class A>
PV_FN bool bgp_is_segment(const A &R, const Parsed &o)
{
    uint32_t pw, hl, fl, plen;
    return bgp_is_segment(R, o, pw, hl, fl, plen);
}
// The segment of such a record: fills g but rec, tcp_sec_before and off; pay_at is the payload's
// first byte in the record blob.
template <class A>
PV_FN bool bgp_segment(const A &R, const Parsed &o, PvBgpSeg &g, uint64_t &pay_at)
{
    uint32_t pw = 0, hl = 0, fl = 0, plen = 0;
    if (!bgp_is_segment(R, o, pw, hl, fl, plen)) return false;
    pay_at = o.l4off + hl;
    const uint64_t cap_end = o.frame + o.caplen;
    const uint64_t avail = cap_end > pay_at ? cap_end - pay_at : 0;
    g.sec = (uint32_t)o.sec;
    g.nsec = (uint32_t)o.nsec;
    g.fkey = flowkey(R, o);
    g.seq = __builtin_bswap32(R.u32(o.l4off + 4));
    g.plen = plen;
    g.caplen = plen > avail ? (uint32_t)avail : plen;
    g.sport = (uint16_t)(((pw & 0xff) << 8) | ((pw >> 8) & 0xff));
    g.dport = (uint16_t)(((pw >> 8) & 0xff00) | (pw >> 24));
    const bool v6first = o.has6 && (!o.has4 || o.v6 < o.v4);
    g.flags = (uint8_t)(fl | (v6first ? PV_BGP_F_V6 : 0u));
    for (int k = 0; k < 7; k++) g.pad[k] = 0;
    const uint64_t a = v6first ? o.v6 + 8 : o.v4 + 12;
    for (uint32_t k = 0; k < 16; k++) g.src[k] = (k < 4 || v6first) ? (uint8_t)R.u8(a + k) : (uint8_t)0;
    return true;
}
#endif // PV_FN

#if defined(__cplusplus) && !defined(PV_BGP_NO_MANAGER)
// ------------------------------------------------------------------ host manager
#include <deque>
#include <list>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "pv_dhcp.h" // pvdhcp::Jsf32, the managers' deep-sampling generator

namespace pvbgp {

enum { C_EVENTS, C_DEEP, C_OPEN, C_UPDATE, C_NOTIFICATION, C_KEEPALIVE, C_ROUTEREFRESH, C_TOTAL, C_FILTERED, C_N };

// BgpMetricsBucket (BgpStreamHandler.h:29-94): the base event counts and the seven counters
struct Bucket {
    int64_t start_sec = 0, start_nsec = 0, end_sec = 0, end_nsec = 0;
    bool read_only = false;
    uint64_t period_length = 0;
    uint64_t c[C_N] = {};
};

struct Stamp {
    int64_t sec = 0, nsec = 0;
};

// One event of the manager, kept on request for the tests (set_event_log)
struct Event {
    int64_t sec, nsec;
    uint32_t type; // byte 18 of the delivered chunk
    uint32_t len;  // the chunk's length
};

// BgpMetricsManager over the segment list: PcapPlusPlus's TcpReassembly as PcapInputStream drives
// it (removeConnInfo, maxOutOfOrderFragments 50, a 30 s LRU time-out), restricted to port-179
// connections; each chunk it delivers is BgpStreamHandler::tcp_message_ready_cb's one event
// (BgpStreamHandler.cpp:75-113,252-284) on the manager's own window (AbstractMetricsManager.h:276-333).
class Manager {
  public:
    Manager(uint32_t num_periods, uint32_t deep_sample_rate);
    // a fresh handler and a fresh input: buckets, generator, connections, the TCP clock
    void reset();
    bool started() const { return started_; }
    void set_start(int64_t sec, int64_t nsec);
    void set_end(int64_t sec, int64_t nsec);
    void check_period_shift(int64_t sec, int64_t nsec);
    // n segments of one batch in record order; payload bytes at arena + off
    void replay(const PvBgpSeg *seg, size_t n, const uint8_t *arena, size_t arena_bytes);
    // the batch is over: tcp_sec is the greatest seconds value of its TCP records (0: none). Runs
    // the time-outs that value causes and carries it into the next batch.
    void end_batch(uint32_t tcp_sec);
    // TcpReassembly::closeAllConnections (the end of the capture)
    void close_all();
    bool window(uint32_t period, bool merged, Bucket &out, std::string &err) const;
    size_t periods() const { return buckets_.size(); }
    size_t open_connections() const { return lru_.size(); }
    size_t known_connections() const { return conns_.size(); }
    // the "bgp" object of window_json: {"period":{...},"wire_packets":{...}}
    static std::string json(const Bucket &b);
    void set_event_log(bool on) { log_on_ = on; }
    const std::vector<Event> &event_log() const { return log_; }

  private:
    struct Frag {
        uint32_t seq;
        std::vector<uint8_t> data;
    };
    struct Side {
        uint8_t ip[16] = {0};
        bool v6 = false, fin = false;
        uint16_t port = 0;
        uint32_t seq = 0;
        std::vector<Frag> frags;
    };
    struct Conn {
        Side side[2];
        int nsides = 0, prev = -1;
        bool closed = false;
        int64_t close_sec = 0;
        Stamp end; // ConnectionData::endTime, {0,0} until the connection's second packet
    };
    typedef std::list<std::pair<uint32_t, Stamp>> Lru;
    void new_event(int64_t sec, int64_t nsec);
    void shift(int64_t sec, int64_t nsec);
    void segment(const PvBgpSeg &g, const uint8_t *data);
    void deliver(uint32_t fk, Conn &c, const uint8_t *d, size_t n);
    void check_ooo(uint32_t fk, Conn &c, int side, bool clean);
    void fin_rst(uint32_t fk, Conn &c, int side, bool rst);
    void close(uint32_t fk);
    void cleanup(int64_t sec);
    void lru_put(uint32_t fk, Stamp t);
    void lru_erase(uint32_t fk);

    uint32_t num_periods_, rate_;
    std::deque<Bucket> buckets_; // front = live
    int64_t next_shift_sec_ = 0;
    bool started_ = false, deep_now_ = true;
    pvdhcp::Jsf32 rng_;
    std::map<uint32_t, Conn> conns_; // by flow key (closeAllConnections visits them in ascending key)
    Lru lru_;                        // front = most recently put
    std::unordered_map<uint32_t, Lru::iterator> lru_at_;
    int64_t now_sec_ = 0;     // the clock a close is stamped with
    uint32_t tcp_sec_max_ = 0; // greatest TCP second of the batches before this one
    bool log_on_ = false;
    std::vector<Event> log_;
};

} // namespace pvbgp
#endif
