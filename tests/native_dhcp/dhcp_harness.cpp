// tests/native_dhcp/dhcp_harness.cpp — TEST ONLY: compiles the DHCP handler's decoder
// (pktvisor_amd/csrc/pv_dhcp.h, the code the HIP kernels run) and its host manager
// (pv_dhcp.cpp) for the CPU behind a small C entry: records in, events and JSON out. Not a
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
#include "../../pktvisor_amd/csrc/pv_dhcp.h"

namespace {

struct HAcc {
    const uint8_t *R;
    uint32_t u32(uint64_t off) const { uint32_t v; memcpy(&v, R + off, 4); return v; }
    uint32_t u32a(uint64_t off) const { return u32(off); }
    uint32_t u8(uint64_t off) const { return R[off]; }
};

// a record's bytes may be followed by anything: the product guarantees PV_RECS_PAD readable
// bytes past the last record, the harness gives each record a copy of its own with 8 (what an
// unaligned word load at a record's last byte can touch), so a sanitizer sees every longer read
const size_t REC_PAD = 8;

struct Harness {
    uint32_t linktype, ts_nano, topn, pct;
    pvdhcp::Manager mgr;
    std::vector<PvDhcpEvent> ev;
    std::vector<uint8_t> arena;
    Harness(uint32_t lt, uint32_t ns, uint32_t periods, uint32_t rate, uint32_t ttl, uint32_t topn_, uint32_t pct_)
        : linktype(lt), ts_nano(ns), topn(topn_), pct(pct_), mgr(periods, rate, ttl) {}
    // decode a block of classic-pcap records; first: the first record's stamp
    size_t decode(const uint8_t *recs, size_t bytes, int64_t first[2])
    {
        ev.clear();
        arena.clear();
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
            if (const uint32_t fam = dhcp_family(R, o)) {
                PvDhcpEvent e;
                uint64_t host_at = 0;
                dhcp_decode(R, linktype, o, fam, (uint32_t)n, e, host_at);
                if (e.family == 4 && e.mtype == 3 && e.host_len) {
                    e.host_off = (uint32_t)arena.size();
                    arena.insert(arena.end(), copy + host_at, copy + host_at + e.host_len);
                }
                ev.push_back(e);
            }
            free(copy);
            pos += len;
            n++;
        }
        return n;
    }
};

} // namespace

extern "C" {

void *dh_new(uint32_t linktype, uint32_t ts_nano, uint32_t periods, uint32_t rate, uint32_t ttl_ms, uint32_t topn, uint32_t pct)
{
    return new Harness(linktype, ts_nano, periods, rate, ttl_ms, topn, pct);
}
void dh_free(void *h) { delete (Harness *)h; }
void dh_reset(void *h) { ((Harness *)h)->mgr.reset(); }

// events of a block of records, without the manager: returns their number; *out stays valid until
// the next call on h, *arena / *arena_bytes the REQUEST hostnames
uint32_t dh_decode(void *hp, const uint8_t *recs, size_t bytes, const PvDhcpEvent **out, const uint8_t **arena, uint32_t *arena_bytes)
{
    Harness *h = (Harness *)hp;
    int64_t first[2] = {0, 0};
    h->decode(recs, bytes, first);
    *out = h->ev.data();
    *arena = h->arena.data();
    *arena_bytes = (uint32_t)h->arena.size();
    return (uint32_t)h->ev.size();
}

// one batch, as pv_process_device feeds the manager: the start stamp is the batch's first record
void dh_feed(void *hp, const uint8_t *recs, size_t bytes)
{
    Harness *h = (Harness *)hp;
    int64_t first[2] = {0, 0};
    if (!h->decode(recs, bytes, first)) return;
    h->mgr.set_start(first[0], first[1]);
    h->mgr.replay(h->ev.data(), h->ev.size(), h->arena.data(), h->arena.size());
}
void dh_set_end(void *h, int64_t sec, int64_t nsec) { ((Harness *)h)->mgr.set_end(sec, nsec); }
void dh_check_period_shift(void *h, int64_t sec, int64_t nsec) { ((Harness *)h)->mgr.check_period_shift(sec, nsec); }
uint32_t dh_periods(void *h) { return (uint32_t)((Harness *)h)->mgr.periods(); }
uint32_t dh_open_transactions(void *h) { return (uint32_t)((Harness *)h)->mgr.open_transactions(); }

// {"dhcp": {...}} of bucket `period` (merged: the fold of the `period` newest), or "!<error>"; free with dh_free_str
char *dh_json(void *hp, uint32_t period, int merged)
{
    Harness *h = (Harness *)hp;
    pvdhcp::Bucket b;
    std::string err;
    if (!h->mgr.window(period, merged != 0, b, err)) return strdup(("!" + err).c_str());
    return strdup(("{\"dhcp\":" + pvdhcp::Manager::json(b, h->topn, h->pct) + "}").c_str());
}
// the bucket's start and end stamps: sec, nsec, sec, nsec
int dh_stamps(void *hp, uint32_t period, int64_t out[4])
{
    Harness *h = (Harness *)hp;
    pvdhcp::Bucket b;
    std::string err;
    if (!h->mgr.window(period, false, b, err)) return -1;
    out[0] = b.start_sec; out[1] = b.start_nsec; out[2] = b.end_sec; out[3] = b.end_nsec;
    return 0;
}
void dh_free_str(char *s) { free(s); }
}
