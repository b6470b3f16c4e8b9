// SPDX-License-Identifier: MPL-2.0
// pv_flow.cpp — the flow handler's host manager: FlowStreamHandler::process_netflow_cb,
// FlowMetricsManager / FlowMetricsBucket (src/handlers/flow/FlowStreamHandler.cpp:393-460,
// 1056-1451,1499-1504) restated over the two ordered lists the device stage (pv_flow.hip) produces.
// Plain C++: needs no GPU, so the CPU tests drive this exact source through tests/native_flow.
//
// Our definitions where the reference has none that a replay can keep:
//   - a datagram whose header time fields are both 0 is stamped with its record's pcap stamp (the
//     reference takes the wall clock);
//   - an IPv4 address is valid unless it is 0.0.0.0 (PcapPlusPlus 23.09's IPv4Address::isValid; not
//     vendored, so unpinned);
//   - top-N lists are exact weighted sums per rendered key, ties ordered by name.
#include "pv_flow.h"

#include "pv_cpc.h"
#include "pv_dhcp.h" // pvdhcp::Manager::top: the host top-N selection rule

#include <algorithm>
#include <arpa/inet.h>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace pvflow {

namespace {

// MurmurHash3_x64_128 with datasketches' DEFAULT_SEED (9001), as cpc_sketch::update(void*, size) runs it
inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
inline uint64_t fmix64(uint64_t k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
    return k;
}
void murmur128(const void *key, size_t len, uint64_t &o1, uint64_t &o2)
{
    const uint64_t c1 = 0x87c37b91114253d5ULL, c2 = 0x4cf5ad432745937fULL;
    const uint8_t *data = (const uint8_t *)key;
    uint64_t h1 = 9001, h2 = 9001;
    const size_t nblocks = len / 16;
    for (size_t i = 0; i < nblocks; i++) {
        uint64_t k1, k2;
        memcpy(&k1, data + 16 * i, 8);
        memcpy(&k2, data + 16 * i + 8, 8);
        k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
        h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
        k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
        h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
    }
    const uint8_t *tail = data + nblocks * 16;
    uint64_t k1 = 0, k2 = 0;
    const size_t r = len & 15;
    for (size_t i = r; i > 8; i--) k2 |= (uint64_t)tail[i - 1] << (8 * (i - 9));
    if (r > 8) { k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2; }
    for (size_t i = std::min<size_t>(r, 8); i > 0; i--) k1 |= (uint64_t)tail[i - 1] << (8 * (i - 1));
    if (r > 0) { k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1; }
    h1 ^= (uint64_t)len; h2 ^= (uint64_t)len;
    h1 += h2; h2 += h1;
    h1 = fmix64(h1); h2 = fmix64(h2);
    h1 += h2; h2 += h1;
    o1 = h1; o2 = h2;
}
// row_col_from_two_hashes (cpc_sketch_impl.hpp:175-185), lg_k = 11
uint32_t coupon_of(const void *key, size_t len)
{
    uint64_t h1, h2;
    murmur128(key, len, h1, h2);
    uint32_t col = h2 ? (uint32_t)__builtin_clzll(h2) : 63;
    if (col > 63) col = 63;
    return ((uint32_t)(h1 & 2047) << 6) | col;
}

std::string ip4_text(uint32_t wire)
{
    char b[20];
    snprintf(b, sizeof b, "%u.%u.%u.%u", wire & 0xff, (wire >> 8) & 0xff, (wire >> 16) & 0xff, wire >> 24);
    return b;
}

// Tos.h:13-36,63-68
std::string dscp_name(uint32_t v)
{
    static const std::map<uint32_t, const char *> names = {
        {0, "CS0"}, {8, "CS1"}, {16, "CS2"}, {24, "CS3"}, {32, "CS4"}, {40, "CS5"}, {48, "CS6"}, {56, "CS7"},
        {10, "AF11"}, {12, "AF12"}, {14, "AF13"}, {18, "AF21"}, {20, "AF22"}, {22, "AF23"}, {26, "AF31"}, {28, "AF32"},
        {30, "AF33"}, {34, "AF41"}, {36, "AF42"}, {38, "AF43"}, {46, "EF"}, {43, "VOICE-ADMIT"}};
    auto it = names.find(v);
    return it != names.end() ? std::string(it->second) : std::to_string(v);
}
std::string ecn_name(uint32_t v)
{
    static const char *names[4] = {"Not-ECT", "ECT(1)", "ECT(0)", "CE"};
    return names[v & 3];
}

void json_str(std::string &s, const std::string &v)
{
    s += '"';
    for (unsigned char c : v) {
        if (c == '"') s += "\\\"";
        else if (c == '\\') s += "\\\\";
        else if (c < 0x20 || c >= 0x80) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); s += b; }
        else s += (char)c;
    }
    s += '"';
}

// TopN::update (src/Metrics.h:543-551): frequent_items_sketch::update ignores a weight of 0
inline void top_add(Top &t, const std::string &key, uint64_t w) { if (w) t[key] += w; }

void member(std::string &s, const char *name)
{
    if (s.back() != '{') s += ',';
    s += '"';
    s += name;
    s += "\":";
}
void top_json(std::string &s, const std::string &name, const Top &t, size_t topn, uint32_t pct)
{
    member(s, name.c_str());
    s += '[';
    bool sep = false;
    for (auto &kv : pvdhcp::Manager::top(t, topn, pct)) {
        if (sep) s += ',';
        sep = true;
        s += "{\"name\":";
        json_str(s, kv.first);
        s += ",\"estimate\":" + std::to_string(kv.second) + "}";
    }
    s += ']';
}

const char *const DIR_NAME[N_DIR] = {"in", "out", "in", "out"};
inline const char *metric_of(int type) { return type == IN_BYTES || type == OUT_BYTES ? "bytes" : "packets"; }

void merge_top(Top &into, const Top &o) { for (auto &kv : o) into[kv.first] += kv.second; }

} // namespace

double sketch_estimate(const Sketch &k, bool merged)
{
    if (merged) return pvh::icon11((uint32_t)k.order.size());
    std::vector<std::pair<int64_t, uint32_t>> f;
    f.reserve(k.order.size());
    for (size_t i = 0; i < k.order.size(); i++) f.push_back({(int64_t)i, k.order[i]});
    return pvh::cpc_hip(f);
}

uint32_t coupon_u32(uint32_t v) { const int64_t x = (int64_t)(int32_t)v; return coupon_of(&x, 8); }
uint32_t coupon_u16(uint16_t v) { const int64_t x = (int64_t)(int16_t)v; return coupon_of(&x, 8); }
uint32_t coupon_str(const std::string &s) { return coupon_of(s.data(), s.size()); }

void PortNames::add(const PortRow &r) { list_[r.udp ? 1 : 0].insert({r.last, {r.name, r.first}}); }

// IpPort::get_service (src/IpPort.cpp:14-32): lower_bound on the rows' last ports; the row found is
// taken when its key is the port or when the port is not below the row's first port
std::string PortNames::service(uint16_t port, bool udp) const
{
    const auto &m = list_[udp ? 1 : 0];
    auto it = m.lower_bound(port);
    if (it == m.end()) return std::to_string(port);
    if (it->first == port || port >= it->second.second) return it->second.first;
    return std::to_string(port);
}

Manager::Manager(uint32_t num_periods, uint32_t deep_sample_rate, uint32_t groups, const std::vector<PortRow> &ports)
    : num_periods_(std::max(1u, std::min(num_periods, 10u)))
    , rate_(deep_sample_rate == 0 ? 100u : std::max(1u, std::min(deep_sample_rate, 100u)))
    , groups_(groups)
{
    for (auto &r : ports) ports_.add(r);
    reset();
}

void Manager::reset()
{
    buckets_.clear();
    buckets_.emplace_front();
    rng_ = Jsf32();
    deep_now_ = true;
    started_ = false;
    next_shift_sec_ = 0;
}

void Manager::set_start(int64_t sec, int64_t nsec)
{
    if (started_) return;
    buckets_.front().start_sec = sec;
    buckets_.front().start_nsec = nsec;
    next_shift_sec_ = sec + 60;
    started_ = true;
}

void Manager::set_end(int64_t sec, int64_t nsec)
{
    if (!started_) return;
    Bucket &b = buckets_.front();
    b.end_sec = sec;
    b.end_nsec = nsec;
    b.period_length = (uint64_t)(sec - b.start_sec);
    b.read_only = true;
}

// _period_shift (src/AbstractMetricsManager.h:276-305)
void Manager::shift(int64_t sec, int64_t nsec)
{
    buckets_.emplace_front();
    buckets_[0].start_sec = sec;
    buckets_[0].start_nsec = nsec;
    Bucket &p = buckets_[1];
    p.end_sec = sec;
    p.end_nsec = nsec;
    p.period_length = (uint64_t)(sec - p.start_sec);
    p.read_only = true;
    if (buckets_.size() > num_periods_) buckets_.pop_back();
    next_shift_sec_ = sec + 60;
}

void Manager::check_period_shift(int64_t sec, int64_t nsec)
{
    if (!started_) return;
    if (num_periods_ > 1 && sec >= next_shift_sec_) shift(sec, nsec);
}

// AbstractMetricsManager::new_event (:318-333)
void Manager::new_event(int64_t sec, int64_t nsec)
{
    if (rate_ != 100) deep_now_ = rng_.next() % 100u < rate_;
    if (num_periods_ > 1 && sec >= next_shift_sec_) shift(sec, nsec);
    Bucket &b = buckets_.front();
    b.events++;
    if (deep_now_) b.deep++;
}

// FlowMetricsBucket::process_interface (:1281-1451) for an IPv4 flow record
void Manager::process_interface(Interface &ifc, const PvFlowRecord &f, int type)
{
    const uint64_t agg = (type == IN_BYTES || type == OUT_BYTES) ? f.octets : f.packets;
    if (on(G_COUNTERS)) {
        uint64_t *c = ifc.counters[type];
        c[K_TOTAL] += agg;
        c[K_IPV4] += agg;
        c[f.proto == 17 ? K_UDP : f.proto == 6 ? K_TCP : K_OTHER] += agg;
    }
    if (!deep_now_) return;
    const bool udp = f.proto == 17; // the port-name protocol: UDP for 17, TCP for everything else (:1321-1324)
    std::string src_port = std::to_string(f.sport), dst_port = std::to_string(f.dport);
    if (on(G_TOP_PORTS)) {
        if (f.sport > 0) {
            src_port = ports_.service(f.sport, udp);
            top_add(ifc.top[type][T_SRC_PORT], src_port, agg);
        }
        if (f.dport > 0) {
            dst_port = ports_.service(f.dport, udp);
            top_add(ifc.top[type][T_DST_PORT], dst_port, agg);
        }
    }
    if (on(G_CARDINALITY)) {
        if (f.sport > 0) ifc.card[S_SRC_PORTS].add(coupon_u16(f.sport));
        if (f.dport > 0) ifc.card[S_DST_PORTS].add(coupon_u16(f.dport));
    }
    if (on(G_TOP_TOS)) {
        top_add(ifc.top[type][T_DSCP], dscp_name(f.tos >> 2), agg);
        top_add(ifc.top[type][T_ECN], ecn_name(f.tos & 3), agg);
    }
    std::string app_src, app_dst;
    if (f.src != 0) {
        if (on(G_CARDINALITY)) ifc.card[S_SRC_IPS].add(coupon_u32(f.src));
        const std::string ip = ip4_text(f.src);
        app_src = ip + ":" + src_port;
        if (on(G_TOP_IPS)) top_add(ifc.top[type][T_SRC_IP], ip, agg);
        if (f.sport > 0 && on(G_TOP_IPS_PORTS)) top_add(ifc.top[type][T_SRC_IP_PORT], app_src, agg);
    }
    if (f.dst != 0) {
        if (on(G_CARDINALITY)) ifc.card[S_DST_IPS].add(coupon_u32(f.dst));
        const std::string ip = ip4_text(f.dst);
        app_dst = ip + ":" + dst_port;
        if (on(G_TOP_IPS)) top_add(ifc.top[type][T_DST_IP], ip, agg);
        if (f.dport > 0 && on(G_TOP_IPS_PORTS)) top_add(ifc.top[type][T_DST_IP_PORT], app_dst, agg);
    }
    if (on(G_CONVERSATIONS) && f.sport > 0 && f.dport > 0 && !app_src.empty() && !app_dst.empty()) {
        const std::string conv = app_src > app_dst ? app_dst + "/" + app_src : app_src + "/" + app_dst;
        if (on(G_CARDINALITY)) ifc.card[S_CONVERSATIONS].add(coupon_str(conv));
        top_add(ifc.conversations[(type == IN_BYTES || type == OUT_BYTES) ? 0 : 1], conv, agg);
    }
}

void Manager::replay(const PvFlowPacket *pk, size_t n, const PvFlowRecord *fr, size_t nfr, uint32_t first_base)
{
    for (size_t i = 0; i < n; i++) {
        const PvFlowPacket &p = pk[i];
        // process_netflow_cb (:393-403)
        if (p.time_sec || p.time_nsec) new_event(p.time_sec, p.time_nsec);
        else new_event(p.sec, p.nsec);
        char t[INET6_ADDRSTRLEN] = "";
        inet_ntop(p.family == 6 ? AF_INET6 : AF_INET, p.addr, t, sizeof t);
        // FlowMetricsBucket::process_flow (:1221-1279); a NetFlow record always has both interface indexes
        Device &d = buckets_.front().devices[t];
        const size_t at = (size_t)(p.first - first_base);
        for (size_t j = 0; j < p.count && at + j < nfr; j++) {
            const PvFlowRecord &f = fr[at + j];
            if (on(G_COUNTERS)) d.flows++;
            for (int out = 0; out < 2; out++) {
                const uint32_t idx = out ? f.if_out : f.if_in;
                Interface &ifc = d.interfaces[idx];
                for (int pkts = 0; pkts < 2; pkts++) {
                    if (!on(pkts ? G_BY_PACKETS : G_BY_BYTES)) continue;
                    const int type = (pkts ? IN_PACKETS : IN_BYTES) + out;
                    process_interface(ifc, f, type);
                    if (deep_now_ && on(G_TOP_INTERFACES)) top_add(d.top_if[type], std::to_string(idx), pkts ? f.packets : f.octets);
                }
            }
        }
    }
}

// window_single_json / window_merged_json's period checks and fold, as pvdhcp::Manager::window;
// FlowMetricsBucket::specialized_merge sums the counters and tops and unions the sketches
bool Manager::window(uint32_t period, bool merged, Bucket &out, std::string &err) const
{
    char m[128];
    if (!merged) {
        if (period >= num_periods_) {
            snprintf(m, sizeof m, "invalid metrics period, specify [0, %u]", num_periods_ - 1);
            err = m;
            return false;
        }
        if (period >= buckets_.size()) {
            snprintf(m, sizeof m, "requested metrics period has not yet accumulated, current range is [0, %zu]", buckets_.size() - 1);
            err = m;
            return false;
        }
        out = buckets_[period];
        if (!out.read_only) out.period_length = 0;
        return true;
    }
    if (period <= 1 || period > num_periods_) {
        snprintf(m, sizeof m, "invalid metrics period, specify [2, %u]", num_periods_);
        err = m;
        return false;
    }
    out = Bucket();
    out.merged = true;
    bool first = true;
    for (size_t i = 0; i < buckets_.size() && i < period; i++) {
        const Bucket &o = buckets_[i];
        out.events += o.events;
        out.deep += o.deep;
        out.period_length += o.read_only ? o.period_length : 0;
        if (first || o.start_sec < out.start_sec) { out.start_sec = o.start_sec; out.start_nsec = o.start_nsec; }
        if (o.end_sec > out.end_sec) { out.end_sec = o.end_sec; out.end_nsec = o.end_nsec; }
        first = false;
        for (auto &dv : o.devices) {
            Device &d = out.devices[dv.first];
            d.flows += dv.second.flows;
            d.filtered += dv.second.filtered;
            for (int k = 0; k < N_DIR; k++) merge_top(d.top_if[k], dv.second.top_if[k]);
            for (auto &iv : dv.second.interfaces) {
                Interface &ifc = d.interfaces[iv.first];
                const Interface &src = iv.second;
                for (int k = 0; k < N_DIR; k++) {
                    for (int q = 0; q < N_KIND; q++) ifc.counters[k][q] += src.counters[k][q];
                    for (int q = 0; q < N_TOP; q++) merge_top(ifc.top[k][q], src.top[k][q]);
                }
                for (int k = 0; k < N_SKETCH; k++)
                    for (uint32_t cp : src.card[k].order) ifc.card[k].add(cp);
                for (int k = 0; k < 2; k++) merge_top(ifc.conversations[k], src.conversations[k]);
            }
        }
    }
    return true;
}

// FlowMetricsBucket::to_json (:1056-1219) with its group gating; object members in the order the
// reference writes them (its JSON library sorts them; consumers must not depend on the order)
std::string Manager::json(const Bucket &b, size_t topn, uint32_t pct) const
{
    static const char *kind_name[N_KIND] = {"udp_", "tcp_", "other_l4_", "ipv4_", "ipv6_", ""};
    static const char *top_name[N_TOP] = {"src_ips", "dst_ips", "src_ports", "dst_ports", "src_ip_ports", "dst_ip_ports", "dscp", "ecn"};
    static const char *card_name[N_SKETCH] = {"conversations", "src_ips_in", "dst_ips_out", "src_ports_in", "dst_ports_out"};
    std::string s = "{\"period\":{\"start_ts\":" + std::to_string(b.start_sec) + ",\"length\":" + std::to_string(b.period_length) +
                    "},\"wire_packets\":{\"events\":" + std::to_string(b.events) + ",\"deep_samples\":" + std::to_string(b.deep) + "}";
    std::string devs = "{";
    for (auto &dv : b.devices) {
        const Device &d = dv.second;
        std::string ds = "{";
        if (on(G_COUNTERS)) {
            member(ds, "records_flows");
            ds += std::to_string(d.flows);
            member(ds, "records_filtered");
            ds += std::to_string(d.filtered);
        }
        if (on(G_TOP_INTERFACES))
            for (int pkts = 0; pkts < 2; pkts++) {
                if (!on(pkts ? G_BY_PACKETS : G_BY_BYTES)) continue;
                for (int out = 0; out < 2; out++) {
                    const int type = (pkts ? IN_PACKETS : IN_BYTES) + out;
                    top_json(ds, std::string("top_") + DIR_NAME[type] + "_interfaces_" + metric_of(type), d.top_if[type], topn, pct);
                }
            }
        std::string ifs = "{";
        for (auto &iv : d.interfaces) {
            const Interface &ifc = iv.second;
            std::string is = "{";
            if (on(G_CARDINALITY)) {
                member(is, "cardinality");
                is += '{';
                for (int k = on(G_CONVERSATIONS) ? 0 : 1; k < N_SKETCH; k++) {
                    member(is, card_name[k]);
                    is += std::to_string(lround(sketch_estimate(ifc.card[k], b.merged)));
                }
                is += '}';
            }
            for (int type = 0; type < N_DIR; type++) {
                if (!on((type == IN_BYTES || type == OUT_BYTES) ? G_BY_BYTES : G_BY_PACKETS) || !on(G_COUNTERS)) continue;
                for (int q = 0; q < N_KIND; q++) {
                    member(is, (std::string(DIR_NAME[type]) + "_" + kind_name[q] + metric_of(type)).c_str());
                    is += std::to_string(ifc.counters[type][q]);
                }
            }
            for (int type = 0; type < N_DIR; type++) {
                if (!on((type == IN_BYTES || type == OUT_BYTES) ? G_BY_BYTES : G_BY_PACKETS)) continue;
                for (int q = 0; q < N_TOP; q++) {
                    const uint32_t g = q < 2 ? G_TOP_IPS : q < 4 ? G_TOP_PORTS : q < 6 ? G_TOP_IPS_PORTS : G_TOP_TOS;
                    if (!on(g)) continue;
                    top_json(is, std::string("top_") + DIR_NAME[type] + "_" + top_name[q] + "_" + metric_of(type), ifc.top[type][q], topn, pct);
                }
            }
            // top_geo (:1186-1216): no database can be attached to this handler while the group is on, so
            // _process_geo_metrics never updates them, and TopN::to_json still writes the four lists, empty
            for (int pkts = 0; pkts < 2; pkts++) {
                if (!on(pkts ? G_BY_PACKETS : G_BY_BYTES)) continue;
                const char *metric = pkts ? "packets" : "bytes";
                if (on(G_TOP_GEO)) {
                    static const Top none;
                    top_json(is, std::string("top_geo_loc_") + metric, none, topn, pct);
                    top_json(is, std::string("top_asn_") + metric, none, topn, pct);
                }
                if (on(G_CONVERSATIONS)) top_json(is, std::string("top_conversations_") + metric, ifc.conversations[pkts], topn, pct);
            }
            if (is.size() == 1) continue;
            is += '}';
            if (ifs.size() > 1) ifs += ',';
            json_str(ifs, std::to_string(iv.first));
            ifs += ':' + is;
        }
        if (ifs.size() > 1) {
            member(ds, "interfaces");
            ds += ifs + '}';
        }
        if (ds.size() == 1) continue;
        ds += '}';
        if (devs.size() > 1) devs += ',';
        json_str(devs, dv.first);
        devs += ':' + ds;
    }
    if (devs.size() > 1) s += ",\"devices\":" + devs + '}';
    s += '}';
    return s;
}

} // namespace pvflow
