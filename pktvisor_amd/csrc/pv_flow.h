// SPDX-License-Identifier: MPL-2.0
// pv_flow.h — the flow handler (src/handlers/flow, src/inputs/flow in the reference) for the
// three fixed-layout, stateless NetFlow export formats (v1, v5, v7): the two lists the device
// stage produces, the datagram check and decoder shared by the device kernels and the CPU test
// harness, and the host manager that replays the lists.
//
// Split, as for DHCP (pv_dhcp.h): whether a record is a flow datagram, and how many flow records
// it carries, is decided from that record's bytes alone, so the device stage (pv_flow.hip) looks at
// every record of a batch; what it finds has strictly sequential semantics (period shifts on the
// manager's own events, one jsf32 draw per datagram, maps that grow in stream order), so the host
// manager (pv_flow.cpp) replays it in record order.
//
// Decode rounds: a round stores the datagrams whose first flow record has a rank in
// [fbase, fbase + cap); a datagram that begins in the round is stored whole, so the record buffer
// has PV_FLOW_SLACK = 29 records of slack behind its cap and no datagram is ever split.
//
// The decoder part needs pv_parse.h included first (it is compiled only when PV_FN is defined);
// the manager part is plain C++.
#pragma once
#include <stdint.h>

#define PV_FLOW_MAX_PORTS 8u
#define PV_FLOW_MAXFLOWS 30u // the largest NFx_MAXFLOWS (3rd/netflow/netflow.h:63,91,121)
#define PV_FLOW_SLACK (PV_FLOW_MAXFLOWS - 1u)

// One accepted datagram, written at its rank among the batch's datagrams (record order)
struct PvFlowPacket {
    uint32_t rec;                // record index in the batch
    uint32_t sec, nsec;          // the record's own stamp (nsec at the record's precision)
    uint32_t time_sec, time_nsec; // the NetFlow header's time_sec / time_nanosec, host order
    uint32_t first;              // rank of its first flow record among the batch's flow records
    uint16_t version, count;
    uint8_t family;              // 4 / 6: the exporter address's family
    uint8_t pad[3];
    uint8_t addr[16];            // exporter address, wire order (4 or 16 bytes)
};
static_assert(sizeof(PvFlowPacket) == 48 && sizeof(PvFlowPacket) % 16 == 0, "PvFlowPacket: 48 bytes");

// One flow record, at its rank (wire order within its datagram). Addresses as loaded from the wire
// (a little-endian load of the network-order bytes), everything else in host order.
struct PvFlowRecord {
    uint32_t src, dst;
    uint32_t packets, octets;
    uint16_t sport, dport;
    uint16_t if_in, if_out;
    uint8_t proto, tos;
    uint8_t pad[6];
};
static_assert(sizeof(PvFlowRecord) == 32, "PvFlowRecord: 32 bytes");

// the configured UDP destination ports (n == 0: any UDP packet), passed to the kernels by value
struct PvFlowPorts {
    uint32_t n;
    uint32_t port[PV_FLOW_MAX_PORTS];
};

#ifdef PV_FN
// ------------------------------------------------------------------ datagram check and decoder
PV_FN uint32_t flow_bswap16(uint32_t v) { return ((v & 0xff) << 8) | ((v >> 8) & 0xff); }
PV_FN uint32_t flow_bswap32(uint32_t v) { return (v << 24) | ((v & 0xff00) << 8) | ((v >> 8) & 0xff00) | (v >> 24); }

// pw: the UDP header's first word, little-endian load
PV_FN bool flow_port_ok(const PvFlowPorts &L, uint32_t pw)
{
    if (!L.n) return true; // the reference's pcap_file mode: every UDP packet (FlowInputStream.cpp:102-109)
    const uint32_t dp = ((pw >> 8) & 0xff00) | (pw >> 24);
    bool ok = false;
#pragma unroll
    for (uint32_t k = 0; k < PV_FLOW_MAX_PORTS; k++) ok = ok || (k < L.n && L.port[k] == dp);
    return ok;
}

// process_netflow_packet's acceptance (NetflowData.h:59-213,678-699) of a UDP payload of plen bytes
// whose first four bytes are hw (little-endian load; not read when plen < 4): the number of flow
// records, 0 = refused. version: the common header's (0 with fewer than four bytes).
PV_FN uint32_t flow_check(uint32_t hw, uint32_t plen, uint32_t &version)
{
    version = 0;
    if (plen < 4) return 0;
    version = flow_bswap16(hw & 0xffff);
    const uint32_t count = flow_bswap16(hw >> 16);
    uint32_t hdr, rec, maxn;
    if (version == 1) { hdr = 16; rec = 48; maxn = 24; }
    else if (version == 5) { hdr = 24; rec = 48; maxn = 30; }
    else if (version == 7) { hdr = 24; rec = 52; maxn = 30; }
    else return 0;
    if (count == 0 || count > maxn || plen != hdr + count * rec) return 0;
    return count;
}

// A parsed record: is it a UDP packet on a configured port (cand), and if so how many flow records
// does its payload [l4off + 8, l4off + l4len), clipped to the captured bytes, carry (0 = invalid)
template <class A>
PV_FN uint32_t flow_classify(const A &R, const Parsed &o, const PvFlowPorts &L, bool &cand, uint32_t &version)
{
    cand = false;
    version = 0;
    if (o.l4 != 17 || o.l4len < 8) return 0;
    if (!flow_port_ok(L, R.u32(o.l4off))) return 0;
    cand = true;
    const uint64_t pay = o.l4off + 8, cap_end = o.frame + o.caplen;
    uint32_t plen = o.l4len - 8;
    const uint64_t avail = cap_end > pay ? cap_end - pay : 0;
    if (plen > avail) plen = (uint32_t)avail;
    if (plen < 4) return 0;
    return flow_check(R.u32(pay), plen, version);
}

// The datagram's entry. Exporter address as FlowInputStream.cpp:110-115 takes it: the source of
// the packet's first IPv4 header, else of its first IPv6 header.
template <class A>
PV_FN void flow_decode_packet(const A &R, const Parsed &o, uint32_t rec, uint32_t version, uint32_t count, uint32_t first,
                              PvFlowPacket &p)
{
    const uint64_t pay = o.l4off + 8;
    p.rec = rec;
    p.sec = (uint32_t)o.sec;
    p.nsec = (uint32_t)o.nsec;
    p.time_sec = flow_bswap32(R.u32(pay + 8));
    p.time_nsec = flow_bswap32(R.u32(pay + 12));
    p.first = first;
    p.version = (uint16_t)version;
    p.count = (uint16_t)count;
    p.family = o.has4 ? 4 : 6;
    for (int k = 0; k < 3; k++) p.pad[k] = 0;
    for (int k = 0; k < 16; k++) p.addr[k] = 0;
    if (o.has4) {
        const uint32_t a = R.u32(o.v4 + 12);
        for (uint32_t k = 0; k < 4; k++) p.addr[k] = (uint8_t)(a >> (8 * k));
    } else if (o.has6) {
        for (uint32_t q = 0; q < 4; q++) {
            const uint32_t a = R.u32(o.v6 + 8 + 4 * q);
            for (uint32_t k = 0; k < 4; k++) p.addr[4 * q + k] = (uint8_t)(a >> (8 * k));
        }
    }
}

// byte offset of flow record j in a datagram of this version (NFx_PACKET_SIZE(j))
PV_FN uint32_t flow_record_at(uint32_t version, uint32_t j) { return (version == 1 ? 16u : 24u) + j * (version == 7 ? 52u : 48u); }

// One wire record (NF1_FLOW / NF5_FLOW / NF7_FLOW share the layout of every field taken: protocol
// at byte 38 and tos at byte 39 in all three)
template <class A>
PV_FN void flow_decode_record(const A &R, uint64_t at, PvFlowRecord &r)
{
    r.src = R.u32(at);
    r.dst = R.u32(at + 4);
    const uint32_t ifw = R.u32(at + 12), pw = R.u32(at + 32), tw = R.u32(at + 36);
    r.if_in = (uint16_t)flow_bswap16(ifw & 0xffff);
    r.if_out = (uint16_t)flow_bswap16(ifw >> 16);
    r.packets = flow_bswap32(R.u32(at + 16));
    r.octets = flow_bswap32(R.u32(at + 20));
    r.sport = (uint16_t)flow_bswap16(pw & 0xffff);
    r.dport = (uint16_t)flow_bswap16(pw >> 16);
    r.proto = (uint8_t)(tw >> 16);
    r.tos = (uint8_t)(tw >> 24);
    for (int k = 0; k < 6; k++) r.pad[k] = 0;
}
#endif // PV_FN

#if defined(__cplusplus) && !defined(PV_FLOW_NO_MANAGER)
// ------------------------------------------------------------------ host manager
#include <deque>
#include <map>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

namespace pvflow {

// group bits (pv_flow_group in include/pvgpu.h)
enum { G_COUNTERS = 1, G_CARDINALITY = 2, G_TOP_IPS = 4, G_TOP_PORTS = 8, G_TOP_IPS_PORTS = 16, G_BY_BYTES = 32,
       G_BY_PACKETS = 64, G_CONVERSATIONS = 128, G_TOP_TOS = 256, G_TOP_GEO = 512, G_TOP_INTERFACES = 1024 };

// FlowDirectionType (FlowStreamHandler.h:47-52)
enum { IN_BYTES, OUT_BYTES, IN_PACKETS, OUT_PACKETS, N_DIR };
// Counters (FlowStreamHandler.h:168-184)
enum { K_UDP, K_TCP, K_OTHER, K_IPV4, K_IPV6, K_TOTAL, N_KIND };
// FlowDirectionTopN (FlowStreamHandler.h:135-155)
enum { T_SRC_IP, T_DST_IP, T_SRC_PORT, T_DST_PORT, T_SRC_IP_PORT, T_DST_IP_PORT, T_DSCP, T_ECN, N_TOP };
// the interface's sketches (FlowStreamHandler.h:188-192)
enum { S_CONVERSATIONS, S_SRC_IPS, S_DST_IPS, S_SRC_PORTS, S_DST_PORTS, N_SKETCH };

// A CPC sketch (lg_k = 11) kept sparsely: its coupons in first-occurrence order
struct Sketch {
    std::vector<uint32_t> order;
    std::unordered_set<uint32_t> seen;
    void add(uint32_t coupon) { if (seen.insert(coupon).second) order.push_back(coupon); }
};

typedef std::map<std::string, uint64_t> Top; // exact weighted sums per rendered key

struct Interface {
    uint64_t counters[N_DIR][N_KIND] = {};
    Sketch card[N_SKETCH];
    Top top[N_DIR][N_TOP];
    Top conversations[2]; // bytes, packets
};

struct Device {
    uint64_t flows = 0, filtered = 0;
    Top top_if[N_DIR];
    std::map<uint32_t, Interface> interfaces;
};

struct Bucket {
    int64_t start_sec = 0, start_nsec = 0, end_sec = 0, end_nsec = 0;
    bool read_only = false, merged = false;
    uint64_t period_length = 0;
    uint64_t events = 0, deep = 0;
    std::map<std::string, Device> devices;
};

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

// IpPort's two port lists (src/IpPort.cpp:11-32): key = a row's last port
struct PortRow {
    uint16_t last, first;
    uint8_t udp; // 1 = the udp list, 0 = the tcp list
    std::string name;
};
class PortNames {
  public:
    void add(const PortRow &r); // std::map::insert: the first row of a key stays
    std::string service(uint16_t port, bool udp) const; // IpPort::get_service
    bool empty() const { return list_[0].empty() && list_[1].empty(); }

  private:
    std::map<uint16_t, std::pair<std::string, uint16_t>> list_[2];
};

// CPC coupons of the items as datasketches' typed cpc_sketch::update overloads hash them
uint32_t coupon_u32(uint32_t v);          // update(uint32_t): the int32 value widened to int64
uint32_t coupon_u16(uint16_t v);          // update(uint16_t): the int16 value widened to int64
uint32_t coupon_str(const std::string &s); // update(const std::string&): its bytes; empty: no update
// the sketch's estimate before rounding: cpc_hip over the first-occurrence order, or, for a sketch
// that is a union of buckets' sketches (merged), icon11 over the number of coupons
double sketch_estimate(const Sketch &k, bool merged);

// FlowMetricsManager over the two lists (FlowStreamHandler.cpp:393-460,1221-1451,1499-1504) with
// its own window (AbstractMetricsManager::new_event / _period_shift)
class Manager {
  public:
    Manager(uint32_t num_periods, uint32_t deep_sample_rate, uint32_t groups, const std::vector<PortRow> &ports);
    void reset();
    bool started() const { return started_; }
    void set_start(int64_t sec, int64_t nsec);
    void set_end(int64_t sec, int64_t nsec);
    void check_period_shift(int64_t sec, int64_t nsec);
    // n datagrams in record order; the flow records of datagram i at fr[pk[i].first - first_base]
    void replay(const PvFlowPacket *pk, size_t n, const PvFlowRecord *fr, size_t nfr, uint32_t first_base);
    bool window(uint32_t period, bool merged, Bucket &out, std::string &err) const;
    size_t periods() const { return buckets_.size(); }
    uint32_t groups() const { return groups_; }
    const PortNames &port_names() const { return ports_; }
    // the "flow" object of window_json
    std::string json(const Bucket &b, size_t topn_count, uint32_t topn_percentile_threshold) const;

  private:
    bool on(uint32_t g) const { return (groups_ & g) != 0; }
    void new_event(int64_t sec, int64_t nsec);
    void shift(int64_t sec, int64_t nsec);
    void process_interface(Interface &ifc, const PvFlowRecord &f, int type);
    uint32_t num_periods_, rate_, groups_;
    PortNames ports_;
    std::deque<Bucket> buckets_; // front = live
    int64_t next_shift_sec_ = 0;
    bool started_ = false, deep_now_ = true;
    Jsf32 rng_;
};

} // namespace pvflow
#endif
