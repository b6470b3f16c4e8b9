// tests/native_bgp/bgp_harness.cpp — TEST ONLY: compiles the BGP handler's segment extraction
// (pktvisor_amd/csrc/pv_bgp.h, the code the HIP kernels run) and its host manager (pv_bgp.cpp)
// for the CPU behind a small C entry: records in, segments, events and JSON out. Not a
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
#include "../../pktvisor_amd/csrc/pv_bgp.h"

namespace {

struct HAcc {
    const uint8_t *R;
    uint32_t u32(uint64_t off) const { uint32_t v; memcpy(&v, R + off, 4); return v; }
    uint32_t u32a(uint64_t off) const { return u32(off); }
    uint32_t u8(uint64_t off) const { return R[off]; }
};

// Each record is decoded from a copy of its own, followed by `pad` bytes: 8 by default (as
// tests/native_dhcp), none after bg_set_pad(0): the sanitizer run's exact-size copies, which show
// any read past a record's captured bytes.
struct Harness {
    uint32_t linktype, ts_nano;
    size_t pad = 8;
    pvbgp::Manager mgr;
    std::vector<PvBgpSeg> seg;
    std::vector<uint8_t> arena;
    uint32_t tcp_sec = 0; // greatest TCP second of the block just extracted
    Harness(uint32_t lt, uint32_t ns, uint32_t periods, uint32_t rate) : linktype(lt), ts_nano(ns), mgr(periods, rate)
    {
        mgr.set_event_log(true);
    }
    // the segments of a block of classic-pcap records, as the device stage gives them for a batch
    size_t extract(const uint8_t *recs, size_t bytes, int64_t first[2])
    {
        seg.clear();
        arena.clear();
        tcp_sec = 0;
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
            uint8_t *copy = (uint8_t *)malloc(len + pad);
            memcpy(copy, recs + pos, len);
            memset(copy + len, 0xA5, pad);
            const HAcc R{copy};
            Parsed o;
            parse_record(R, C, P, 0, o);
            PvBgpSeg g;
            uint64_t pay_at = 0;
            if (bgp_segment(R, o, g, pay_at)) {
                g.rec = (uint32_t)n;
                g.tcp_sec_before = tcp_sec;
                g.off = (uint32_t)arena.size();
                arena.insert(arena.end(), copy + pay_at, copy + pay_at + g.caplen);
                seg.push_back(g);
            }
            if (bgp_is_tcp(o) && (uint32_t)o.sec > tcp_sec) tcp_sec = (uint32_t)o.sec;
            free(copy);
            pos += len;
            n++;
        }
        return n;
    }
};

} // namespace

extern "C" {

void *bg_new(uint32_t linktype, uint32_t ts_nano, uint32_t periods, uint32_t rate) { return new Harness(linktype, ts_nano, periods, rate); }
void bg_free(void *h) { delete (Harness *)h; }
void bg_reset(void *h) { ((Harness *)h)->mgr.reset(); }
void bg_set_pad(void *h, uint32_t pad) { ((Harness *)h)->pad = pad; }

// segments of a block of records, without the manager: returns their number; *out stays valid
// until the next call on h, *arena / *arena_bytes their payload bytes
uint32_t bg_extract(void *hp, const uint8_t *recs, size_t bytes, const PvBgpSeg **out, const uint8_t **arena, uint32_t *arena_bytes)
{
    Harness *h = (Harness *)hp;
    int64_t first[2] = {0, 0};
    h->extract(recs, bytes, first);
    *out = h->seg.data();
    *arena = h->arena.data();
    *arena_bytes = (uint32_t)h->arena.size();
    return (uint32_t)h->seg.size();
}

// one batch, as pv_process_device feeds the manager: the start stamp is the batch's first record;
// eoc: the capture's final batch
void bg_feed(void *hp, const uint8_t *recs, size_t bytes, int eoc)
{
    Harness *h = (Harness *)hp;
    int64_t first[2] = {0, 0};
    if (!h->extract(recs, bytes, first)) return;
    h->mgr.set_start(first[0], first[1]);
    h->mgr.replay(h->seg.data(), h->seg.size(), h->arena.data(), h->arena.size());
    h->mgr.end_batch(h->tcp_sec);
    if (eoc) h->mgr.close_all();
}
void bg_set_end(void *h, int64_t sec, int64_t nsec) { ((Harness *)h)->mgr.set_end(sec, nsec); }
void bg_check_period_shift(void *h, int64_t sec, int64_t nsec) { ((Harness *)h)->mgr.check_period_shift(sec, nsec); }
uint32_t bg_periods(void *h) { return (uint32_t)((Harness *)h)->mgr.periods(); }
uint32_t bg_open_connections(void *h) { return (uint32_t)((Harness *)h)->mgr.open_connections(); }
uint32_t bg_known_connections(void *h) { return (uint32_t)((Harness *)h)->mgr.known_connections(); }

// the manager's events so far (since the last reset): sec, nsec, type, length
uint32_t bg_events(void *hp, const pvbgp::Event **out)
{
    Harness *h = (Harness *)hp;
    *out = h->mgr.event_log().data();
    return (uint32_t)h->mgr.event_log().size();
}

// {"bgp": {...}} of bucket `period` (merged: the fold of the `period` newest), or "!<error>"; free with bg_free_str
char *bg_json(void *hp, uint32_t period, int merged)
{
    Harness *h = (Harness *)hp;
    pvbgp::Bucket b;
    std::string err;
    if (!h->mgr.window(period, merged != 0, b, err)) return strdup(("!" + err).c_str());
    return strdup(("{\"bgp\":" + pvbgp::Manager::json(b) + "}").c_str());
}
// the bucket's start and end stamps: sec, nsec, sec, nsec
int bg_stamps(void *hp, uint32_t period, int64_t out[4])
{
    Harness *h = (Harness *)hp;
    pvbgp::Bucket b;
    std::string err;
    if (!h->mgr.window(period, false, b, err)) return -1;
    out[0] = b.start_sec; out[1] = b.start_nsec; out[2] = b.end_sec; out[3] = b.end_nsec;
    return 0;
}
void bg_free_str(char *s) { free(s); }
}
