// tests/native/parse_harness.cpp — TEST ONLY: compiles the product's parse/decode
// source (pktvisor_amd/csrc/pv_parse.h, the code the HIP kernel runs) for the CPU
// so it can be fuzzed against the oracle without a GPU. Not a fallback: nothing in
// the product loads this library.
#include <cstring>
#include <stdint.h>

#define PV_FN inline
#define PV_CREF(T) const T &
inline uint32_t pv_clz64(uint64_t x) { return (uint32_t)__builtin_clzll(x); }
inline uint32_t pv_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh)); }
#include "../../pktvisor_amd/csrc/pv_parse.h"

// plain-memory accessor (the kernel uses an LDS-window accessor with the same interface)
struct HAcc {
    const uint8_t *R;
    uint32_t u32(uint64_t off) const { uint32_t v; memcpy(&v, R + off, 4); return v; }
    uint32_t u32a(uint64_t off) const { return u32(off); }
    uint32_t u8(uint64_t off) const { return R[off]; }
};

extern "C" {

// first query name of a DNS message (buffer must be readable 8 bytes past len):
// returns m_NameLength, writes the raw name bytes (as the final std::string) to out
uint32_t h_decode_qname(const uint8_t *msg, uint32_t len, char *out, uint32_t *outlen)
{
    struct Coll {
        char *o;
        uint32_t n;
        void put(uint32_t c) { o[n++] = (char)c; }
    } col{out, 0};
    const HAcc R{msg};
    uint32_t nl = name_len_l1(R, 0, len, 12);
    if (nl > 0) name_emit(R, 0, len, 12, col);
    *outlen = col.n;
    return nl;
}

// parseResources(queryOnly) outcome: ok, has_query, qtype
void h_dns_parse(const uint8_t *msg, uint32_t len, int *ok, int *has_query, uint32_t *qtype)
{
    DnsInfo d;
    const HAcc R{msg};
    uint32_t qd = be16(R, 4), an = be16(R, 6), ns = be16(R, 8), ar = be16(R, 10);
    dns_parse(R, 0, len, qd, an, ns, ar, d);
    *ok = d.ok; *has_query = d.has_query; *qtype = d.qtype;
}

// lower-case name stats: length, murmur (CPC) halves, aggregateDomain suffix starts
void h_name_stats(const uint8_t *msg, uint32_t len, uint32_t *n, uint64_t *h1, uint64_t *h2, int *q2, int *q3)
{
    NameStats st;
    st.init();
    const HAcc R{msg};
    uint32_t nl = name_len_l1(R, 0, len, 12);
    if (nl > 0) name_emit(R, 0, len, 12, st);
    *n = st.n;
    st.mm.finish(*h1, *h2);
    uint64_t a, b;
    if (st.n) agg_domain(st, *q2, *q3, a, b); else { *q2 = 0; *q3 = -1; }
}
}

extern "C" {
// name_stats_fast against name_emit + NameStats on the same message:
// -1 = the fast path declined, 1 = every NameStats field equal, 0 = a field differs
int h_name_fast_check(const uint8_t *msg, uint32_t len)
{
    const HAcc R{msg};
    uint32_t nl = name_len_l1(R, 0, len, 12);
    if (nl == 0) return -1;
    NameStats a, b;
    a.init();
    b.init();
    if (!name_stats_fast(R, 0, len, 12, a)) return -1;
    name_emit(R, 0, len, 12, b);
    uint64_t a1, a2, b1, b2;
    a.mm.finish(a1, a2);
    b.mm.finish(b1, b2);
    return a1 == b1 && a2 == b2 && a.ph == b.ph && a.n == b.n && a.last_c == b.last_c && a.d0 == b.d0 &&
           a.d1 == b.d1 && a.d2 == b.d2 && a.d3 == b.d3 && a.h0 == b.h0 && a.h1 == b.h1 && a.h2 == b.h2 &&
           a.h3 == b.h3;
}
}

// plain-memory accessor that records how far its reads went: the end of the highest byte read,
// with a word read counted as its four bytes
struct TrAcc {
    const uint8_t *R;
    uint64_t *hi;
    void note(uint64_t end) const { if (end > *hi) *hi = end; }
    uint32_t u32(uint64_t off) const { note(off + 4); uint32_t v; memcpy(&v, R + off, 4); return v; }
    uint32_t u32a(uint64_t off) const { return u32(off); }
    uint32_t u8(uint64_t off) const { note(off + 1); return R[off]; }
};

// The 12 header bytes the way the kernels' dns_header takes them: bytes past the message read as 0
static uint32_t hdr16(const uint8_t *msg, uint32_t len, uint32_t off)
{
    return ((off < len ? msg[off] : 0u) << 8) | (off + 1 < len ? msg[off + 1] : 0u);
}

// Every DNS entry point of pv_parse.h on one message, through one accessor. v[PV_DNS_ALL_VALS]:
// name_len_l1; dns_parse ok, has_query, qtype, name_len_enc; NameStats n, murmur halves, the
// aggregateDomain starts; the fast path's verdict (h_name_fast_check's); dns_dnssec;
// dns_first_additional; dns_ecs family and address. name: name_emit's bytes.
#define PV_DNS_ALL_VALS 15
template <class A>
static void dns_all(const A &R, const uint8_t *msg, uint32_t len, uint64_t *v, char *name, uint32_t *name_n)
{
    struct Coll {
        char *o;
        uint32_t n;
        void put(uint32_t c) { o[n++] = (char)c; }
    } col{name, 0};
    const uint32_t qd = hdr16(msg, len, 4), an = hdr16(msg, len, 6), ns = hdr16(msg, len, 8), ar = hdr16(msg, len, 10);
    const uint32_t nl = name_len_l1(R, 0, len, 12);
    if (nl > 0) name_emit(R, 0, len, 12, col);
    *name_n = col.n;
    v[0] = nl;
    DnsInfo d;
    dns_parse(R, 0, len, qd, an, ns, ar, d);
    v[1] = d.ok; v[2] = d.has_query; v[3] = d.qtype; v[4] = d.name_len_enc;
    NameStats st, fs;
    st.init();
    fs.init();
    if (nl > 0) name_emit(R, 0, len, 12, st);
    v[5] = st.n;
    Murmur mm = st.mm;
    mm.finish(v[6], v[7]);
    int q2 = 0, q3 = -1;
    uint64_t a, b;
    if (st.n) agg_domain(st, q2, q3, a, b);
    v[8] = (uint64_t)(int64_t)q2; v[9] = (uint64_t)(int64_t)q3;
    v[10] = (uint64_t)(int64_t)-1;
    if (nl > 0 && name_stats_fast(R, 0, len, 12, fs)) {
        uint64_t f1, f2;
        fs.mm.finish(f1, f2);
        v[10] = f1 == v[6] && f2 == v[7] && fs.ph == st.ph && fs.n == st.n && fs.last_c == st.last_c && fs.d0 == st.d0 &&
                fs.d1 == st.d1 && fs.d2 == st.d2 && fs.d3 == st.d3 && fs.h0 == st.h0 && fs.h1 == st.h1 && fs.h2 == st.h2 &&
                fs.h3 == st.h3;
    }
    v[11] = dns_dnssec(R, 0, len, qd, an, ns, ar);
    v[12] = dns_first_additional(R, 0, len, qd, an, ns, ar);
    uint64_t addr = 0;
    v[13] = dns_ecs(R, 0, len, qd, an, ns, ar, addr);
    v[14] = addr;
}

extern "C" {
// the message must be readable PV_RECS_PAD bytes past len, as every record blob on the device is
int h_dns_dnssec(const uint8_t *msg, uint32_t len)
{
    const HAcc R{msg};
    return dns_dnssec(R, 0, len, hdr16(msg, len, 4), hdr16(msg, len, 6), hdr16(msg, len, 8), hdr16(msg, len, 10));
}
// offset of the first additional record, 0 if none
uint32_t h_first_additional(const uint8_t *msg, uint32_t len)
{
    const HAcc R{msg};
    return dns_first_additional(R, 0, len, hdr16(msg, len, 4), hdr16(msg, len, 6), hdr16(msg, len, 8), hdr16(msg, len, 10));
}
// ECS family (0 none, 1 IPv4, 2 IPv6) and the kept address bytes, little-endian
uint32_t h_dns_ecs(const uint8_t *msg, uint32_t len, uint64_t *addr)
{
    const HAcc R{msg};
    return dns_ecs(R, 0, len, hdr16(msg, len, 4), hdr16(msg, len, 6), hdr16(msg, len, 8), hdr16(msg, len, 10), *addr);
}
void h_dns_all(const uint8_t *msg, uint32_t len, uint64_t *v, char *name, uint32_t *name_n)
{
    const HAcc R{msg};
    dns_all(R, msg, len, v, name, name_n);
}
// the same through TrAcc: returns the end of the highest byte read (0: nothing was read)
uint64_t h_dns_all_tracked(const uint8_t *msg, uint32_t len, uint64_t *v, char *name, uint32_t *name_n)
{
    uint64_t hi = 0;
    const TrAcc R{msg, &hi};
    dns_all(R, msg, len, v, name, name_n);
    return hi;
}
}

#include <arpa/inet.h>

// PvParams::nets from subnet lists, as pv_host.cpp fills it from a host spec (v4: in_addr.s_addr
// and CIDR; v6: 16 address bytes and CIDR)
static void fill_nets(PvSubnets &s, uint32_t n4, const uint32_t *v4_addr, const uint32_t *v4_cidr, uint32_t n6,
                      const uint8_t *v6_addr, const uint32_t *v6_cidr)
{
    memset(&s, 0, sizeof s);
    for (uint32_t i = 0; i < n4 && i < PV_MAX_SUBNETS; i++) {
        const uint32_t k = s.n4++;
        s.v4_addr[k] = v4_addr[i];
        s.v4_all[k] = v4_cidr[i] == 0;
        s.v4_mask[k] = v4_cidr[i] == 0 ? 0 : htonl(0xFFFFFFFFu << (32 - v4_cidr[i]));
    }
    for (uint32_t i = 0; i < n6 && i < PV_MAX_SUBNETS; i++) {
        memcpy(s.v6_addr[s.n6], v6_addr + 16 * i, 16);
        s.v6_cidr[s.n6++] = v6_cidr[i];
    }
}

// one row of PV_PARSE_COLS values per record: l3, l4, has4, has6, syn, dir, v4, v6, l4off, l4len;
// the three offsets relative to frame byte 0, -1 where the layer is absent
#define PV_PARSE_COLS 10
template <class A>
static void parse_row(const A &R, const PvParams &P, uint64_t rec, int64_t *row)
{
    Parsed o;
    parse_record(R, P, rec, o);
    row[0] = o.l3; row[1] = o.l4; row[2] = o.has4; row[3] = o.has6; row[4] = o.syn; row[5] = o.dir;
    row[6] = o.has4 ? (int64_t)(o.v4 - o.frame) : -1;
    row[7] = o.has6 ? (int64_t)(o.v6 - o.frame) : -1;
    row[8] = o.l4 ? (int64_t)(o.l4off - o.frame) : -1;
    row[9] = o.l4len;
}

extern "C" {
// parse_record over a blob of classic-pcap records (16-byte header + caplen bytes each; the blob
// readable 8 bytes past len). Returns the number of rows written (at most max_rows).
uint64_t h_parse_records(const uint8_t *blob, uint64_t len, uint32_t linktype, uint32_t ts_nano, uint32_t n4,
                         const uint32_t *v4_addr, const uint32_t *v4_cidr, uint32_t n6, const uint8_t *v6_addr,
                         const uint32_t *v6_cidr, int64_t *rows, uint64_t max_rows)
{
    PvParams P;
    memset(&P, 0, sizeof P);
    P.linktype = linktype;
    P.ts_nano = ts_nano;
    fill_nets(P.nets, n4, v4_addr, v4_cidr, n6, v6_addr, v6_cidr);
    const HAcc R{blob};
    uint64_t pos = 0, n = 0;
    while (pos + 16 <= len && n < max_rows) {
        const uint32_t cap = R.u32(pos + 8);
        if (pos + 16 + cap > len) break;
        parse_row(R, P, pos, rows + PV_PARSE_COLS * n++);
        pos += 16 + (uint64_t)cap;
    }
    return n;
}
}

#ifdef PV_PARSE_BOUNDED
// Accessor for the stand-alone sanitizer program (parse_asan_main.cpp): the record lives in a heap
// block of exactly its own size. A byte read goes to memory as it is, so one past the block is a
// sanitizer report. A word read is how the kernels fetch a 16-bit field (one LDS word, the upper
// bytes masked off), so it may straddle the end by design: its bytes inside the block are read,
// those past it are taken from `fill`. The program parses every record under two fills and the two
// rows must be equal, so a result that depends on a byte past the record is a finding either way.
struct BAcc {
    const uint8_t *R;
    uint64_t end;
    uint8_t fill;
    uint32_t u32(uint64_t off) const
    {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; k++) v |= (uint32_t)(off + k < end ? R[off + k] : fill) << (8 * k);
        return v;
    }
    uint32_t u32a(uint64_t off) const { return u32(off); }
    uint32_t u8(uint64_t off) const { return R[off]; }
};
extern "C" void h_parse_bounded(const uint8_t *rec, uint64_t size, uint8_t fill, uint32_t linktype, uint32_t n4,
                                const uint32_t *v4_addr, const uint32_t *v4_cidr, uint32_t n6, const uint8_t *v6_addr,
                                const uint32_t *v6_cidr, int64_t *row)
{
    PvParams P;
    memset(&P, 0, sizeof P);
    P.linktype = linktype;
    fill_nets(P.nets, n4, v4_addr, v4_cidr, n6, v6_addr, v6_cidr);
    const BAcc R{rec, size, fill};
    parse_row(R, P, 0, row);
}
#endif
