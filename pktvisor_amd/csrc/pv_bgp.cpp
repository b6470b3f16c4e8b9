// SPDX-License-Identifier: MPL-2.0
// pv_bgp.cpp — the BGP handler's host manager: BgpMetricsManager / BgpMetricsBucket
// (src/handlers/bgp/BgpStreamHandler.cpp:75-113,215-284, .h:29-106) behind PcapPlusPlus's
// TcpReassembly as PcapInputStream drives it (PcapInputStream.cpp:75-79,254-283,429-465),
// restated over the ordered segment list the device stage (pv_bgp.hip) produces. Plain C++:
// needs no GPU, so the CPU tests drive this exact source through tests/native_bgp.
#include "pv_bgp.h"

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "pv_layout.h" // PV_TCP_RECLAIM

namespace pvbgp {

namespace {

const size_t MAX_OOO = 50;     // TcpReassemblyConfiguration::maxOutOfOrderFragments as the input sets it
const int64_t TCP_TIMEOUT = 30; // PcapInputStream.h:97

bool seq_lt(uint32_t a, uint32_t b) { return (int32_t)(a - b) < 0; }
bool seq_gt(uint32_t a, uint32_t b) { return (int32_t)(b - a) < 0; }

} // namespace

Manager::Manager(uint32_t num_periods, uint32_t deep_sample_rate)
    : num_periods_(std::max(1u, std::min(num_periods, 10u)))
    , rate_(deep_sample_rate == 0 ? 100u : std::max(1u, std::min(deep_sample_rate, 100u)))
{
    reset();
}

void Manager::reset()
{
    buckets_.clear();
    buckets_.emplace_front();
    rng_ = pvdhcp::Jsf32();
    deep_now_ = true;
    started_ = false;
    next_shift_sec_ = 0;
    conns_.clear();
    lru_.clear();
    lru_at_.clear();
    now_sec_ = 0;
    tcp_sec_max_ = 0;
    log_.clear();
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

// _period_shift (:276-305); the BGP manager has no on_period_shift work
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
    b.c[C_EVENTS]++;
    if (deep_now_) b.c[C_DEEP]++;
}

// VisorLRUList as the input uses it: put moves the key to the front with a new time
void Manager::lru_put(uint32_t fk, Stamp t)
{
    lru_erase(fk);
    lru_.emplace_front(fk, t);
    lru_at_[fk] = lru_.begin();
}
void Manager::lru_erase(uint32_t fk)
{
    auto it = lru_at_.find(fk);
    if (it == lru_at_.end()) return;
    lru_.erase(it->second);
    lru_at_.erase(it);
}

// onMessageReady -> tcp_message_ready_cb: one parseBgpLayer call on the chunk, which reads its
// first message only. The type is byte 18; a chunk without one, or with a type outside 1..5,
// is no event (the reference dereferences a null layer there: our definition). Then the input's
// LRU put with the connection's endTime.
void Manager::deliver(uint32_t fk, Conn &c, const uint8_t *d, size_t n)
{
    const uint32_t type = n >= 19 ? d[18] : 0u;
    if (type >= 1 && type <= 5) {
        new_event(c.end.sec, c.end.nsec);
        Bucket &b = buckets_.front();
        b.c[C_TOTAL]++;
        b.c[C_OPEN + (type - 1)]++;
        if (log_on_) log_.push_back(Event{c.end.sec, c.end.nsec, type, (uint32_t)n});
    }
    lru_put(fk, c.end);
}

// checkOutOfOrderFragments: deliver held fragments that have become in order (or overlap what was
// delivered) until none is; with `clean`, or with more than 50 held, the fragment of the lowest
// sequence goes out behind a "[N bytes missing]" text and the search starts over
void Manager::check_ooo(uint32_t fk, Conn &c, int side, bool clean)
{
    Side &s = c.side[side];
    bool found;
    do {
        do {
            found = false;
            size_t i = 0;
            while (i < s.frags.size()) {
                if (s.frags[i].seq == s.seq) {
                    std::vector<uint8_t> d = std::move(s.frags[i].data);
                    s.frags.erase(s.frags.begin() + i);
                    s.seq += (uint32_t)d.size();
                    deliver(fk, c, d.data(), d.size());
                    found = true;
                } else if (seq_lt(s.frags[i].seq, s.seq)) {
                    const uint32_t fseq = s.frags[i].seq;
                    std::vector<uint8_t> d = std::move(s.frags[i].data);
                    s.frags.erase(s.frags.begin() + i);
                    if (seq_gt(fseq + (uint32_t)d.size(), s.seq)) {
                        const uint32_t skip = s.seq - fseq;
                        s.seq += (uint32_t)d.size() - skip;
                        deliver(fk, c, d.data() + skip, d.size() - skip);
                        found = true;
                    }
                } else i++;
            }
        } while (found);
        if (!clean && s.frags.size() <= MAX_OOO) break;
        if (s.frags.empty()) break;
        size_t best = 0;
        for (size_t i = 1; i < s.frags.size(); i++)
            if (seq_lt(s.frags[i].seq, s.frags[best].seq)) best = i;
        Frag f = std::move(s.frags[best]);
        s.frags.erase(s.frags.begin() + best);
        char text[40];
        const int tl = snprintf(text, sizeof text, "[%u bytes missing]", f.seq - s.seq);
        s.seq = f.seq + (uint32_t)f.data.size();
        std::vector<uint8_t> d(text, text + tl);
        d.insert(d.end(), f.data.begin(), f.data.end());
        deliver(fk, c, d.data(), d.size());
        found = true;
    } while (found);
}

// closeConnectionInternal: both sides flushed, the connection leaves the LRU list and its key is
// ignored until PV_TCP_RECLAIM event seconds have passed
void Manager::close(uint32_t fk)
{
    auto it = conns_.find(fk);
    if (it == conns_.end() || it->second.closed) return;
    Conn &c = it->second;
    check_ooo(fk, c, 0, true);
    check_ooo(fk, c, 1, true);
    lru_erase(fk);
    c.closed = true;
    c.close_sec = now_sec_;
    for (Side &s : c.side) std::vector<Frag>().swap(s.frags);
}

// handleFinOrRst
void Manager::fin_rst(uint32_t fk, Conn &c, int side, bool rst)
{
    if (c.side[side].fin) return;
    c.side[side].fin = true;
    if (c.side[1 - side].fin || rst) close(fk);
    else check_ooo(fk, c, side, true);
}

// PcapInputStream's clean-up after a TCP packet of second `sec` (the cap of 100 per packet is not
// modelled): connections whose last put is 30 s old are closed from the tail of the LRU list
void Manager::cleanup(int64_t sec)
{
    now_sec_ = sec;
    while (!lru_.empty()) {
        const std::pair<uint32_t, Stamp> back = lru_.back();
        if (sec < back.second.sec + TCP_TIMEOUT) break;
        close(back.first);
        lru_erase(back.first);
    }
}

// TcpReassembly::reassemblePacket on one segment (pv_bgp.h bgp_segment has applied the TcpLayer
// and "no data, no flag" rules); data: its captured payload, g.caplen bytes (== g.plen: parse_record
// trims the layer to the captured bytes)
void Manager::segment(const PvBgpSeg &g, const uint8_t *data)
{
    now_sec_ = g.sec;
    const uint32_t fk = g.fkey, plen = g.caplen;
    const bool syn = g.flags & PV_BGP_F_SYN, fin = g.flags & PV_BGP_F_FIN, rst = g.flags & PV_BGP_F_RST, v6 = g.flags & PV_BGP_F_V6;
    const Stamp now{(int64_t)g.sec, (int64_t)(g.nsec / 1000u * 1000u)}; // ConnectionData keeps timevals
    auto it = conns_.find(fk);
    if (it != conns_.end() && it->second.closed) {
        if ((int64_t)g.sec < it->second.close_sec + (int64_t)PV_TCP_RECLAIM) return; // a packet of a closed flow
        conns_.erase(it);
        it = conns_.end();
    }
    if (it == conns_.end()) {
        it = conns_.emplace(fk, Conn()).first;
        lru_put(fk, now); // onConnectionStart
    } else {
        Stamp &e = it->second.end;
        if (now.sec > e.sec || (now.sec == e.sec && now.nsec > e.nsec)) e = now;
    }
    Conn &c = it->second;
    auto is_side = [&](int k) { return c.side[k].port == g.sport && c.side[k].v6 == v6 && !memcmp(c.side[k].ip, g.src, 16); };
    int side;
    bool first = false;
    if (c.nsides < 2 && !(c.nsides == 1 && is_side(0))) {
        side = c.nsides++;
        memcpy(c.side[side].ip, g.src, 16);
        c.side[side].v6 = v6;
        c.side[side].port = g.sport;
        first = true;
    } else if (is_side(0)) side = 0;
    else if (c.nsides == 2 && is_side(1)) side = 1;
    else return; // a third endpoint under the same key
    Side &s = c.side[side];
    if (s.fin) return;
    if ((fin || rst) && plen == 0) { fin_rst(fk, c, side, rst); return; }
    if (c.prev != -1 && c.prev != side) check_ooo(fk, c, c.prev, true); // the side changed
    c.prev = side;
    if (first) {
        s.seq = g.seq + plen + (syn ? 1u : 0u);
        if (plen) deliver(fk, c, data, plen);
    } else if (seq_lt(g.seq, s.seq)) {
        // a retransmission; what reaches past the delivered bytes is new
        if (seq_gt(g.seq + plen, s.seq)) {
            const uint32_t skip = s.seq - g.seq;
            s.seq += plen - skip;
            deliver(fk, c, data + skip, plen - skip);
        }
    } else if (g.seq == s.seq) {
        if (plen) {
            s.seq += plen + (syn ? 1u : 0u);
            deliver(fk, c, data, plen);
            check_ooo(fk, c, side, false);
        }
    } else if (plen) {
        s.frags.push_back(Frag{g.seq, std::vector<uint8_t>(data, data + plen)});
        if (s.frags.size() > MAX_OOO) check_ooo(fk, c, side, true);
    }
    if (fin || rst) fin_rst(fk, c, side, rst);
}

void Manager::replay(const PvBgpSeg *seg, size_t n, const uint8_t *arena, size_t arena_bytes)
{
    static const uint8_t none[1] = {0};
    for (size_t i = 0; i < n; i++) {
        const PvBgpSeg &g = seg[i];
        // the time-outs every TCP record before this one has caused (stamps taken as monotone)
        const uint32_t before = std::max(tcp_sec_max_, g.tcp_sec_before);
        if (before) cleanup(before);
        if (g.caplen && (size_t)g.off + g.caplen > arena_bytes) continue; // (cannot happen: a round fits its arena)
        segment(g, g.caplen ? arena + g.off : none);
        cleanup(g.sec);
    }
}

void Manager::end_batch(uint32_t tcp_sec)
{
    tcp_sec_max_ = std::max(tcp_sec_max_, tcp_sec);
    if (!tcp_sec_max_) return;
    cleanup(tcp_sec_max_);
    // closed connections whose reclaim time has passed are forgotten here, not only when their key
    // comes again: a tap that sees port-179 probes from ever-new sources keeps 300 s of them
    for (auto it = conns_.begin(); it != conns_.end();) {
        if (it->second.closed && it->second.close_sec + (int64_t)PV_TCP_RECLAIM <= (int64_t)tcp_sec_max_) it = conns_.erase(it);
        else ++it;
    }
}

void Manager::close_all()
{
    std::vector<uint32_t> keys;
    for (auto &kv : conns_)
        if (!kv.second.closed) keys.push_back(kv.first);
    for (uint32_t fk : keys) close(fk);
}

// window_single_json / window_merged_json's period checks and fold (AbstractMetricsManager.h:480-504,
// 601-647; AbstractMetricsBucket::merge :177-195, BgpMetricsBucket::specialized_merge). A live
// bucket of a stream that has not ended has length 0, as the other handlers' outputs have.
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
    }
    return true;
}

// BgpMetricsBucket::to_json (:215-238); rates are timer-driven and not kept
std::string Manager::json(const Bucket &b)
{
    static const char *names[C_N] = {"events", "deep_samples", "open", "update", "notification", "keepalive", "routerefresh", "total",
                                     "filtered"};
    std::string s = "{\"period\":{\"start_ts\":" + std::to_string(b.start_sec) + ",\"length\":" + std::to_string(b.period_length) +
                    "},\"wire_packets\":{";
    for (int k = 0; k < C_N; k++) {
        if (k) s += ',';
        s += '"';
        s += names[k];
        s += "\":" + std::to_string(b.c[k]);
    }
    s += "}}";
    return s;
}

} // namespace pvbgp
