// SPDX-License-Identifier: MPL-2.0
// pv_dhcp.cpp — the DHCP handler's host manager: DhcpMetricsManager / DhcpMetricsBucket
// (src/handlers/dhcp/DhcpStreamHandler.cpp:231-346, .h:41-146) restated over the ordered event
// list the device stage (pv_dhcp.hip) produces. Plain C++: needs no GPU, so the CPU tests drive
// this exact source through tests/native_dhcp.
#include "pv_dhcp.h"

#include <algorithm>
#include <arpa/inet.h>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace pvdhcp {

namespace {

// pcpp message types
enum { DHCP_DISCOVER = 1, DHCP_OFFER = 2, DHCP_REQUEST = 3, DHCP_ACK = 5 };
enum { DHCPV6_SOLICIT = 1, DHCPV6_ADVERTISE = 2, DHCPV6_REQUEST = 3, DHCPV6_REPLY = 7 };

std::string mac_text(const uint8_t *m)
{
    char b[24];
    snprintf(b, sizeof b, "%02x:%02x:%02x:%02x:%02x:%02x", m[0], m[1], m[2], m[3], m[4], m[5]);
    return b;
}
std::string ip4_text(uint32_t wire)
{
    char b[20];
    snprintf(b, sizeof b, "%u.%u.%u.%u", wire & 0xff, (wire >> 8) & 0xff, (wire >> 16) & 0xff, wire >> 24);
    return b;
}

// strings go out as DNS names do (pv_host.h Json::esc): bytes below 0x20 and from 0x80 as \u00XX
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

} // namespace

Manager::Manager(uint32_t num_periods, uint32_t deep_sample_rate, uint32_t xact_ttl_ms)
    : num_periods_(std::max(1u, std::min(num_periods, 10u)))
    , rate_(deep_sample_rate == 0 ? 100u : std::max(1u, std::min(deep_sample_rate, 100u)))
{
    // TransactionManager::TransactionManager (TransactionManager.h:61-69)
    if (xact_ttl_ms == 0) xact_ttl_ms = 5000;
    if (xact_ttl_ms > 1000) {
        ttl_s_ = xact_ttl_ms / 1000;
        ttl_ms_ = xact_ttl_ms - ttl_s_ * 1000;
    } else ttl_ms_ = xact_ttl_ms;
    reset();
}

void Manager::reset()
{
    buckets_.clear();
    buckets_.emplace_front();
    xact_.clear();
    rng_ = Jsf32();
    deep_now_ = true;
    started_ = false;
    next_shift_sec_ = 0;
}

void Manager::set_start(int64_t sec, int64_t nsec)
{
    if (started_) return;
    // AbstractMetricsManager::set_start_tstamp (:423-431)
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

// _period_shift (:276-305) and DhcpMetricsManager::on_period_shift -> purge_old_transactions
// (TransactionManager.h:94-106: seconds only)
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
    for (auto it = xact_.begin(); it != xact_.end();) {
        if (sec >= (int64_t)ttl_s_ + it->second.sec) it = xact_.erase(it);
        else ++it;
    }
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
    b.c[C_EVENTS]++;
    if (deep_now_) b.c[C_DEEP]++;
}

void Manager::replay(const PvDhcpEvent *evs, size_t n, const uint8_t *arena, size_t arena_bytes)
{
    for (size_t i = 0; i < n; i++) {
        const PvDhcpEvent &e = evs[i];
        new_event(e.sec, e.nsec);
        Bucket &b = buckets_.front();
        const bool deep = deep_now_;
        if (e.family == 4) {
            // DhcpMetricsBucket::process_dhcp_layer (:231-266)
            b.c[C_TOTAL]++;
            switch (e.mtype) {
            case DHCP_DISCOVER: b.c[C_DISCOVER]++; break;
            case DHCP_OFFER: b.c[C_OFFER]++; break;
            case DHCP_REQUEST: b.c[C_REQUEST]++; break;
            case DHCP_ACK: b.c[C_ACK]++; break;
            default: break;
            }
            if (deep && e.mtype == DHCP_OFFER && (e.flags & PV_DHCP_F_SERVER) && (e.flags & PV_DHCP_F_ETH))
                b.servers[mac_text(e.emac) + "/" + ip4_text(e.server_id)]++;
            // DhcpMetricsManager::process_dhcp_layer (:318-338)
            if (e.mtype == DHCP_REQUEST) {
                std::string host = "Unknown";
                if (e.flags & PV_DHCP_F_HOST) {
                    host.clear();
                    if (e.host_len && (size_t)e.host_off + e.host_len <= arena_bytes)
                        host.assign(reinterpret_cast<const char *>(arena + e.host_off), e.host_len);
                }
                xact_[e.xid] = Xact{(int64_t)e.sec, (int64_t)e.nsec, std::move(host), mac_text(e.cmac)};
            } else if (e.mtype == DHCP_ACK) {
                auto it = xact_.find(e.xid);
                if (it == xact_.end()) continue;
                // maybe_end_transaction (TransactionManager.h:24-37,76-92)
                const Xact x = std::move(it->second);
                xact_.erase(it);
                int64_t ds = (int64_t)e.sec > x.sec ? (int64_t)e.sec - x.sec : x.sec - (int64_t)e.sec;
                int64_t dn = (int64_t)e.nsec - x.nsec;
                if (dn < 0) { --ds; dn += 1000000000L; }
                const bool timed_out = ds > (int64_t)ttl_s_ || (ds == (int64_t)ttl_s_ && ((double)dn / 1.0e6) >= (double)ttl_ms_);
                // new_dhcp_transaction (:267-278)
                if (!timed_out && deep && e.yiaddr != 0) b.clients[x.mac + "/" + x.hostname + "/" + ip4_text(e.yiaddr)]++;
            }
        } else {
            // DhcpMetricsBucket::process_dhcp_v6_layer (:280-316): no `total`
            switch (e.mtype) {
            case DHCPV6_SOLICIT: b.c[C_SOLICIT]++; break;
            case DHCPV6_ADVERTISE: b.c[C_ADVERTISE]++; break;
            case DHCPV6_REQUEST: b.c[C_REQUEST_V6]++; break;
            case DHCPV6_REPLY: b.c[C_REPLY]++; break;
            default: break;
            }
            static const uint8_t zero16[16] = {};
            if (deep && (e.mtype == DHCPV6_REPLY || e.mtype == DHCPV6_ADVERTISE) && (e.flags & PV_DHCP_F_SERVER) &&
                (e.flags & PV_DHCP_F_ETH) && (e.flags & PV_DHCP_F_V6SRC) && memcmp(e.v6src, zero16, 16) != 0) {
                char t[INET6_ADDRSTRLEN] = "";
                inet_ntop(AF_INET6, e.v6src, t, sizeof t);
                b.servers[mac_text(e.emac) + "/" + t]++;
            }
        }
    }
}

// window_single_json / window_merged_json's period checks and fold (AbstractMetricsManager.h:480-504,
// 601-647; AbstractMetricsBucket::merge :177-195, DhcpMetricsBucket::specialized_merge). A live
// bucket of a stream that has not ended has length 0, as the Net and DNS outputs have.
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
    bool first = true;
    for (size_t i = 0; i < buckets_.size() && i < period; i++) {
        const Bucket &o = buckets_[i];
        for (int k = 0; k < C_N; k++) out.c[k] += o.c[k];
        out.period_length += o.read_only ? o.period_length : 0;
        if (first || o.start_sec < out.start_sec) { out.start_sec = o.start_sec; out.start_nsec = o.start_nsec; }
        if (o.end_sec > out.end_sec) { out.end_sec = o.end_sec; out.end_nsec = o.end_nsec; }
        first = false;
        for (auto &kv : o.clients) out.clients[kv.first] += kv.second;
        for (auto &kv : o.servers) out.servers[kv.first] += kv.second;
    }
    return true;
}

std::vector<std::pair<std::string, uint64_t>> Manager::top(const std::map<std::string, uint64_t> &m, size_t n, uint32_t pct)
{
    std::vector<std::pair<std::string, uint64_t>> v(m.begin(), m.end());
    std::sort(v.begin(), v.end(), [](const auto &a, const auto &b) {
        if (a.second != b.second) return a.second > b.second;
        return a.first < b.first;
    });
    const size_t k = std::min(n, v.size());
    v.resize(k);
    if (!k) return v;
    std::vector<uint64_t> est;
    for (auto &kv : v) est.push_back(kv.second);
    std::sort(est.begin(), est.end());
    const uint64_t w = (uint64_t)std::ceil((double)pct / 100.0 * (double)k);
    const uint64_t thr = est[w == 0 ? 0 : std::min<size_t>(w - 1, k - 1)];
    size_t keep = 0;
    while (keep < k && v[keep].second >= thr) keep++;
    v.resize(keep);
    return v;
}

// DhcpMetricsBucket::to_json (:182-211); rates are timer-driven and not kept
std::string Manager::json(const Bucket &b, size_t topn, uint32_t pct)
{
    static const char *names[C_N] = {"events", "deep_samples", "discover", "offer", "request", "ack", "solicit", "advertise",
                                     "request_v6", "reply", "total", "filtered"};
    std::string s = "{\"period\":{\"start_ts\":" + std::to_string(b.start_sec) + ",\"length\":" + std::to_string(b.period_length) +
                    "},\"wire_packets\":{";
    for (int k = 0; k < C_N; k++) {
        if (k) s += ',';
        s += '"';
        s += names[k];
        s += "\":" + std::to_string(b.c[k]);
    }
    s += '}';
    for (int t = 0; t < 2; t++) {
        s += t ? ",\"top_servers\":[" : ",\"top_clients\":[";
        bool sep = false;
        for (auto &kv : top(t ? b.servers : b.clients, topn, pct)) {
            if (sep) s += ',';
            sep = true;
            s += "{\"name\":";
            json_str(s, kv.first);
            s += ",\"estimate\":" + std::to_string(kv.second) + "}";
        }
        s += ']';
    }
    s += '}';
    return s;
}

} // namespace pvdhcp
