// tests/native_flow/flow_harness.cpp — TEST ONLY: compiles the flow handler's datagram check and
// decoder (pktvisor_amd/csrc/pv_flow.h, the code the HIP kernels run) and its host manager
// (pv_flow.cpp) for the CPU behind a small C entry: records in, the two lists and JSON out. Not a
// fallback: nothing in the product loads this library.
#include <cstdlib>
#include <cstring>
#include <stdint.h>
#include <string>
#include <vector>

#define PV_FN inline
#define PV_CREF(T) const T &
inline uint32_t pv_clz64(uint64_t x) { return (uint32_t)__builtin_clzll(x); }
inline uint32_t pv_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh)); }
#include "../../pktvisor_amd/csrc/pv_parse.h"
#include "../../pktvisor_amd/csrc/pv_flow.h"

namespace {

struct HAcc {
    const uint8_t *R;
    uint32_t u32(uint64_t off) const { uint32_t v; memcpy(&v, R + off, 4); return v; }
    uint32_t u32a(uint64_t off) const { return u32(off); }
    uint32_t u8(uint64_t off) const { return R[off]; }
};

// each record is decoded from a copy of its own with 8 bytes behind it (what an unaligned word
// load at a record's last byte can touch), so a sanitizer sees every longer read
const size_t REC_PAD = 8;

struct Row {
    uint16_t last, first;
    uint32_t protocol;
    const char *name;
};

std::vector<pvflow::PortRow> rows_of(const Row *rows, uint32_t n)
{
    std::vector<pvflow::PortRow> out;
    for (uint32_t k = 0; k < n; k++) out.push_back({rows[k].last, rows[k].first, (uint8_t)(rows[k].protocol == 17), rows[k].name});
    return out;
}

struct Harness {
    uint32_t linktype, ts_nano, topn, pct;
    PvFlowPorts ports;
    pvflow::Manager mgr;
    std::vector<PvFlowPacket> pk;
    std::vector<PvFlowRecord> fr;
    uint64_t stats[3] = {0, 0, 0};
    Harness(uint32_t lt, uint32_t ns, uint32_t periods, uint32_t rate, uint32_t groups, uint32_t topn_, uint32_t pct_,
            const uint16_t *p, uint32_t np, const Row *rows, uint32_t nrows)
        : linktype(lt), ts_nano(ns), topn(topn_), pct(pct_), ports{}, mgr(periods, rate, groups, rows_of(rows, nrows))
    {
        ports.n = np < PV_FLOW_MAX_PORTS ? np : PV_FLOW_MAX_PORTS;
        for (uint32_t k = 0; k < ports.n; k++) ports.port[k] = p[k];
    }
    size_t decode(const uint8_t *recs, size_t bytes, int64_t first[2])
    {
        pk.clear();
        fr.clear();
        PvParams P;
        memset(&P, 0, sizeof P);
        ParseCfg C;
        memset(&C, 0, sizeof C);
        C.linktype = linktype;
        C.ts_nano = ts_nano;
        C.m0 = C.m1 = 0xffffffffu;
        size_t pos = 0, n = 0;
        while (pos + 16 <= bytes) {
            uint32_t h[4];
            memcpy(h, recs + pos, 16);
            if (pos + 16 + (size_t)h[2] > bytes) break;
            if (n == 0) { first[0] = h[0]; first[1] = ts_nano ? (int64_t)h[1] : (int64_t)h[1] * 1000; }
            const size_t len = 16 + (size_t)h[2];
            uint8_t *copy = (uint8_t *)malloc(len + REC_PAD);
            memcpy(copy, recs + pos, len);
            memset(copy + len, 0xA5, REC_PAD);
            const HAcc R{copy};
            Parsed o;
            parse_record(R, C, P, 0, o);
            bool cand = false;
            uint32_t version = 0;
            const uint32_t count = flow_classify(R, o, ports, cand, version);
            if (count) {
                PvFlowPacket p;
                flow_decode_packet(R, o, (uint32_t)n, version, count, (uint32_t)fr.size(), p);
                pk.push_back(p);
                for (uint32_t j = 0; j < count; j++) {
                    PvFlowRecord f;
                    flow_decode_record(R, o.l4off + 8 + flow_record_at(version, j), f);
                    fr.push_back(f);
                }
                stats[0]++;
            } else if (cand) {
                stats[1]++;
                if (version == 9 || version == 10) stats[2]++;
            }
            free(copy);
            pos += len;
            n++;
        }
        return n;
    }
};

char *dup(const std::string &s) { return strdup(s.c_str()); }

} // namespace

extern "C" {

void *fl_new(uint32_t linktype, uint32_t ts_nano, uint32_t periods, uint32_t rate, uint32_t groups, uint32_t topn, uint32_t pct,
             const uint16_t *ports, uint32_t nports, const Row *rows, uint32_t nrows)
{
    return new Harness(linktype, ts_nano, periods, rate, groups, topn, pct, ports, nports, rows, nrows);
}
void fl_free(void *h) { delete (Harness *)h; }

// the two lists of a block of records, without the manager; they stay valid until the next call on h
uint32_t fl_decode(void *hp, const uint8_t *recs, size_t bytes, const PvFlowPacket **pk, const PvFlowRecord **fr, uint32_t *nfr)
{
    Harness *h = (Harness *)hp;
    int64_t first[2] = {0, 0};
    h->decode(recs, bytes, first);
    *pk = h->pk.data();
    *fr = h->fr.data();
    *nfr = (uint32_t)h->fr.size();
    return (uint32_t)h->pk.size();
}

// one batch: the input's start stamp is its first record's; then the replay
void fl_feed(void *hp, const uint8_t *recs, size_t bytes)
{
    Harness *h = (Harness *)hp;
    int64_t first[2] = {0, 0};
    if (!h->decode(recs, bytes, first)) return;
    h->mgr.set_start(first[0], first[1]);
    h->mgr.replay(h->pk.data(), h->pk.size(), h->fr.data(), h->fr.size(), 0);
}
void fl_set_end(void *h, int64_t sec, int64_t nsec) { ((Harness *)h)->mgr.set_end(sec, nsec); }
void fl_check_period_shift(void *h, int64_t sec, int64_t nsec) { ((Harness *)h)->mgr.check_period_shift(sec, nsec); }
uint32_t fl_periods(void *h) { return (uint32_t)((Harness *)h)->mgr.periods(); }
void fl_stats(void *h, uint64_t out[3]) { for (int k = 0; k < 3; k++) out[k] = ((Harness *)h)->stats[k]; }

// {"flow": ...} of a period / the merged window; "!" + the error text when the period is refused
char *fl_json(void *hp, uint32_t period, int merged)
{
    Harness *h = (Harness *)hp;
    pvflow::Bucket b;
    std::string err;
    if (!h->mgr.window(period, merged != 0, b, err)) return dup("!" + err);
    return dup("{\"flow\":" + h->mgr.json(b, h->topn, h->pct) + "}");
}
// the manager's coupon of one item: kind 0 = a u32 (an address), 1 = a u16 (a port), 2 = a string
uint32_t fl_coupon(int kind, uint32_t value, const char *text)
{
    return kind == 0 ? pvflow::coupon_u32(value) : kind == 1 ? pvflow::coupon_u16((uint16_t)value) : pvflow::coupon_str(text);
}
// the unrounded estimate of a sketch fed n items in order (kind 0 / 1: values; kind 2: n strings,
// each ended by a 0 byte, in text); merged: as a union's
double fl_estimate(int kind, const uint32_t *values, const char *text, uint32_t n, int merged)
{
    pvflow::Sketch s;
    for (uint32_t i = 0; i < n; i++) {
        if (kind == 2) {
            const std::string item(text);
            text += item.size() + 1;
            if (!item.empty()) s.add(pvflow::coupon_str(item)); // cpc_sketch::update(const std::string&) skips an empty one
        } else s.add(kind == 0 ? pvflow::coupon_u32(values[i]) : pvflow::coupon_u16((uint16_t)values[i]));
    }
    return pvflow::sketch_estimate(s, merged != 0);
}
char *fl_service(void *hp, uint32_t port, int udp) { return dup(((Harness *)hp)->mgr.port_names().service((uint16_t)port, udp != 0)); }
void fl_free_str(char *s) { free(s); }
}
