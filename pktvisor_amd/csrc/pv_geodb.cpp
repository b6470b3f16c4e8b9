// SPDX-License-Identifier: MPL-2.0
//
// pv_geodb.cpp — MaxMind DB 2.0 reader (see pv_geodb.h). The file is untrusted: every offset is
// checked against the section it indexes, a pointer that lands on a pointer is refused, nesting
// is capped, and every child index of the compiled tree is validated, so neither this reader
// nor the tree walkers (host and device) can leave their arrays.
#include "pv_geodb.h"

#include "../../include/pvgpu.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <tuple>

namespace {

enum : uint32_t {
    T_EXT = 0, T_POINTER = 1, T_STRING = 2, T_DOUBLE = 3, T_BYTES = 4, T_UINT16 = 5, T_UINT32 = 6, T_MAP = 7,
    T_INT32 = 8, T_UINT64 = 9, T_UINT128 = 10, T_ARRAY = 11, T_CACHE = 12, T_END = 13, T_BOOL = 14, T_FLOAT = 15
};

struct Val {
    uint32_t type = 0;
    uint32_t size = 0; // payload bytes; entries of a map / array; the value of a boolean; a pointer's target
    size_t at = 0;     // offset of the payload (containers: of the first member)
};

// One data section (the data records, or the metadata map): pointers are offsets into it.
struct Section {
    const uint8_t *p;
    size_t n;
    std::string *err;

    bool bad(const char *what) const
    {
        if (err->empty()) *err = what;
        return false;
    }

    // control byte(s) at off -> v; off moves to the payload (for a pointer: past it)
    bool head(size_t &off, Val &v) const
    {
        if (off >= n) return bad("data section: value past the end");
        const uint8_t c = p[off++];
        uint32_t type = c >> 5;
        if (type == T_POINTER) {
            const uint32_t ss = (c >> 3) & 3, nb = ss + 1;
            if (n - off < nb) return bad("data section: truncated pointer");
            uint32_t x = ss == 3 ? 0 : (uint32_t)(c & 7);
            for (uint32_t i = 0; i < nb; i++) x = (x << 8) | p[off + i];
            off += nb;
            static const uint32_t add[4] = {0, 2048, 526336, 0};
            v.type = T_POINTER;
            v.size = x + add[ss];
            v.at = off;
            return true;
        }
        if (type == T_EXT) {
            if (off >= n) return bad("data section: truncated extended type");
            type = 7u + p[off++];
            if (type < 8 || type > T_FLOAT) return bad("data section: unknown type");
        }
        uint32_t size = c & 31;
        if (size >= 29) {
            const uint32_t nb = size - 28;
            if (n - off < nb) return bad("data section: truncated size");
            uint32_t x = 0;
            for (uint32_t i = 0; i < nb; i++) x = (x << 8) | p[off + i];
            off += nb;
            size = x + (nb == 1 ? 29u : nb == 2 ? 285u : 65821u);
        }
        v.type = type;
        v.size = size;
        v.at = off;
        if (type == T_MAP || type == T_ARRAY || type == T_BOOL) return true;
        if (type == T_CACHE || type == T_END) return bad("data section: container / end marker as a value");
        if (n - off < size) return bad("data section: payload past the end");
        if ((type == T_DOUBLE && size != 8) || (type == T_FLOAT && size != 4) || (type == T_UINT16 && size > 2) ||
            ((type == T_UINT32 || type == T_INT32) && size > 4) || (type == T_UINT64 && size > 8) ||
            (type == T_UINT128 && size > 16))
            return bad("data section: number of a wrong size");
        return true;
    }

    // off -> just past the value there; pointers are stepped over, not followed
    bool skip(size_t &off, int depth) const
    {
        Val v;
        if (!head(off, v)) return false;
        if (v.type == T_MAP || v.type == T_ARRAY) {
            if (depth >= PV_GEO_MAX_DEPTH) return bad("data section: nested too deep");
            const uint64_t members = (uint64_t)v.size * (v.type == T_MAP ? 2 : 1);
            if (members > n - off) return bad("data section: container larger than the section");
            for (uint64_t i = 0; i < members; i++)
                if (!skip(off, depth + 1)) return false;
            return true;
        }
        if (v.type != T_POINTER && v.type != T_BOOL) off += v.size;
        return true;
    }

    // the value at off, behind at most one pointer (a pointer to a pointer is refused)
    bool value(size_t off, Val &v) const
    {
        if (!head(off, v)) return false;
        if (v.type != T_POINTER) return true;
        size_t t = v.size;
        if (t >= n) return bad("data section: pointer past the end");
        if (!head(t, v)) return false;
        if (v.type == T_POINTER) return bad("data section: pointer to a pointer");
        return true;
    }

    // member `key` of the map m: 1 found (out), 0 absent, -1 malformed
    int member(const Val &m, const char *key, Val &out) const
    {
        if (m.type != T_MAP) return 0;
        const size_t kl = strlen(key);
        size_t off = m.at;
        for (uint32_t i = 0; i < m.size; i++) {
            Val k;
            if (!value(off, k)) return -1;
            if (k.type != T_STRING) return bad("data section: map key is not a string"), -1;
            if (!skip(off, 0)) return -1; // the key (inline or a pointer)
            if (k.size == kl && !memcmp(p + k.at, key, kl)) return value(off, out) ? 1 : -1;
            if (!skip(off, 0)) return -1;
        }
        return 0;
    }

    int element(const Val &a, uint32_t idx, Val &out) const
    {
        if (a.type != T_ARRAY || idx >= a.size) return 0;
        size_t off = a.at;
        for (uint32_t i = 0; i < idx; i++)
            if (!skip(off, 0)) return -1;
        return value(off, out) ? 1 : -1;
    }

    // MMDB_get_value along map keys; "#k" selects element k of an array
    int path(const Val &root, std::initializer_list<const char *> keys, Val &out) const
    {
        Val cur = root;
        for (const char *k : keys) {
            Val nxt;
            const int r = k[0] == '#' ? element(cur, (uint32_t)atoi(k + 1), nxt) : member(cur, k, nxt);
            if (r <= 0) return r;
            cur = nxt;
        }
        out = cur;
        return 1;
    }

    uint64_t uint_of(const Val &v) const
    {
        uint64_t x = 0;
        for (uint32_t i = 0; i < v.size && i < 8; i++) x = (x << 8) | p[v.at + i];
        return x;
    }
    std::string str_of(const Val &v) const { return std::string((const char *)p + v.at, v.size); }
    double double_of(const Val &v) const
    {
        const uint64_t b = uint_of(v);
        double d;
        memcpy(&d, &b, 8);
        return d;
    }
};

// _getGeoLoc (GeoDB.cpp:179-244)
bool render_city(const Section &s, const Val &rec, pv_geodb::Entry &e)
{
    Val v;
    int r;
    if ((r = s.path(rec, {"continent", "code"}, v)) < 0) return false;
    if (r && v.type == T_STRING) e.name += s.str_of(v);
    if ((r = s.path(rec, {"country", "names", "en"}, v)) < 0) return false;
    if (!r && (r = s.path(rec, {"country", "iso_code"}, v)) < 0) return false;
    if (r && v.type == T_STRING) e.name += "/" + s.str_of(v);
    if ((r = s.path(rec, {"subdivisions", "#0", "iso_code"}, v)) < 0) return false;
    if (r && v.type == T_STRING) e.name += "/" + s.str_of(v);
    if ((r = s.path(rec, {"city", "names", "en"}, v)) < 0) return false;
    if (r && v.type == T_STRING) e.name += "/" + s.str_of(v);
    if ((r = s.path(rec, {"location", "latitude"}, v)) < 0) return false;
    if (r && v.type == T_DOUBLE) e.lat = std::to_string(s.double_of(v));
    if ((r = s.path(rec, {"location", "longitude"}, v)) < 0) return false;
    if (r && v.type == T_DOUBLE) e.lon = std::to_string(s.double_of(v));
    return true;
}

// _getASNString (GeoDB.cpp:371-413)
bool render_asn(const Section &s, const Val &rec, pv_geodb::Entry &e)
{
    Val v;
    int r;
    if ((r = s.path(rec, {"autonomous_system_number"}, v)) < 0) return false;
    if (r) {
        if (v.type == T_UINT16 || v.type == T_UINT32 || v.type == T_UINT64) e.name += std::to_string(s.uint_of(v));
        else if (v.type == T_INT32) e.name += std::to_string((int32_t)(uint32_t)s.uint_of(v));
        else if (v.type == T_STRING) e.name += s.str_of(v);
    }
    if ((r = s.path(rec, {"autonomous_system_organization"}, v)) < 0) return false;
    if (r && v.type == T_STRING) e.name += "/" + s.str_of(v);
    return true;
}

const uint8_t MARKER[] = {0xab, 0xcd, 0xef, 'M', 'a', 'x', 'M', 'i', 'n', 'd', '.', 'c', 'o', 'm'};

uint32_t record(const uint8_t *node, uint32_t rs, int side)
{
    if (rs == 24) {
        const uint8_t *b = node + 3 * side;
        return (uint32_t)b[0] << 16 | (uint32_t)b[1] << 8 | b[2];
    }
    if (rs == 28) {
        if (!side) return (uint32_t)(node[3] & 0xf0) << 20 | (uint32_t)node[0] << 16 | (uint32_t)node[1] << 8 | node[2];
        return (uint32_t)(node[3] & 0x0f) << 24 | (uint32_t)node[4] << 16 | (uint32_t)node[5] << 8 | node[6];
    }
    const uint8_t *b = node + 4 * side;
    return (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | b[3];
}

uint64_t fnv(uint64_t h, const void *d, size_t n)
{
    const uint8_t *b = (const uint8_t *)d;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

thread_local std::string g_err;

} // namespace

namespace pvgeo {

pv_geodb *open(const uint8_t *buf, size_t len, uint32_t kind, std::string &err)
{
    err.clear();
    if (!buf || kind > PV_GEODB_ASN) { err = "bad argument"; return nullptr; }
    // the last metadata marker of the file
    size_t mpos = SIZE_MAX;
    if (len >= sizeof MARKER)
        for (size_t i = len - sizeof MARKER + 1; i-- > 0;)
            if (buf[i] == MARKER[0] && !memcmp(buf + i, MARKER, sizeof MARKER)) { mpos = i; break; }
    if (mpos == SIZE_MAX) { err = "not a MaxMind DB file: no metadata marker"; return nullptr; }
    const Section meta{buf + mpos + sizeof MARKER, len - mpos - sizeof MARKER, &err};
    Val root, v;
    size_t whole = 0;
    if (!meta.value(0, root) || !meta.skip(whole, 0)) { err = "metadata: " + err; return nullptr; }
    if (root.type != T_MAP) { err = "metadata is not a map"; return nullptr; }
    uint64_t m[3];
    const char *names[3] = {"node_count", "record_size", "ip_version"};
    for (int i = 0; i < 3; i++) {
        const int r = meta.member(root, names[i], v);
        if (r < 0) { err = "metadata: " + err; return nullptr; }
        if (!r || !(v.type == T_UINT16 || v.type == T_UINT32 || v.type == T_UINT64)) {
            err = std::string("metadata: ") + names[i] + " missing or not an unsigned integer";
            return nullptr;
        }
        m[i] = meta.uint_of(v);
    }
    const uint64_t nc = m[0], rs = m[1], ipv = m[2];
    if (rs != 24 && rs != 28 && rs != 32) { err = "unsupported record_size " + std::to_string(rs); return nullptr; }
    if (ipv != 4 && ipv != 6) { err = "unsupported ip_version " + std::to_string(ipv); return nullptr; }
    const uint64_t node_bytes = rs / 4;
    // (nc is bounded by the file before it is multiplied)
    if (nc > mpos / node_bytes || nc * node_bytes + 16 > mpos || nc >= PV_GEO_LEAF) {
        err = "node_count " + std::to_string(nc) + " does not fit the file";
        return nullptr;
    }
    const size_t tree_bytes = (size_t)(nc * node_bytes);
    const Section data{buf + tree_bytes + 16, mpos - tree_bytes - 16, &err};

    pv_geodb *db = new pv_geodb;
    db->kind = kind;
    db->ip_version = (uint32_t)ipv;
    db->node_count = (uint32_t)nc;
    db->tree.assign((size_t)nc * 2, PV_GEO_LEAF);
    db->dict.push_back({"Unknown", "", ""});

    // every node the root reaches (a malformed tree may share or loop: each node once)
    std::vector<uint8_t> seen((size_t)nc, 0);
    std::vector<uint32_t> stack;
    std::vector<std::pair<uint32_t, size_t>> leaves; // (data offset, tree word)
    if (nc) { stack.push_back(0); seen[0] = 1; }
    while (!stack.empty()) {
        const uint32_t node = stack.back();
        stack.pop_back();
        for (int side = 0; side < 2; side++) {
            const uint32_t r = record(buf + (size_t)node * node_bytes, (uint32_t)rs, side);
            const size_t w = (size_t)node * 2 + side;
            if (r < nc) {
                db->tree[w] = r;
                if (!seen[r]) { seen[r] = 1; stack.push_back(r); }
            } else if (r > nc) {
                const uint64_t doff = (uint64_t)r - nc;
                if (doff < 16 || doff - 16 >= data.n) {
                    err = "search tree: record of node " + std::to_string(node) + " points outside the data section";
                    delete db;
                    return nullptr;
                }
                leaves.emplace_back((uint32_t)(doff - 16), w);
            } // r == nc: no entry, id 0
        }
    }
    // ids in the order of the first data offset that renders each string: a function of the file
    std::sort(leaves.begin(), leaves.end());
    std::map<std::tuple<std::string, std::string, std::string>, uint32_t> ids;
    ids[{"Unknown", "", ""}] = 0;
    uint32_t last_off = 0, last_id = 0;
    bool have = false;
    for (const auto &lf : leaves) {
        if (!have || lf.first != last_off) {
            Val rec;
            size_t end = lf.first;
            pv_geodb::Entry e;
            // the record itself is walked whole once (depth cap), then read along the paths
            if (!data.skip(end, 0) || !data.value(lf.first, rec) ||
                !(kind == PV_GEODB_CITY ? render_city(data, rec, e) : render_asn(data, rec, e))) {
                err = "data record at " + std::to_string(lf.first) + ": " + err;
                delete db;
                return nullptr;
            }
            auto it = ids.find({e.name, e.lat, e.lon});
            if (it == ids.end()) {
                it = ids.emplace(std::make_tuple(e.name, e.lat, e.lon), (uint32_t)db->dict.size()).first;
                db->dict.push_back(e);
            }
            last_off = lf.first;
            last_id = it->second;
            have = true;
        }
        db->tree[lf.second] = PV_GEO_LEAF | last_id;
    }
    uint32_t w = nc ? 0 : PV_GEO_LEAF;
    if (ipv == 6)
        for (int i = 0; i < 96 && !(w & PV_GEO_LEAF); i++) w = db->tree[(size_t)w * 2];
    db->start4 = w;
    uint64_t h = fnv(14695981039346656037ull, db->tree.data(), db->tree.size() * 4);
    const uint32_t hdr[3] = {db->ip_version, db->node_count, db->start4};
    h = fnv(h, hdr, sizeof hdr);
    for (const auto &e : db->dict)
        for (const std::string *s : {&e.name, &e.lat, &e.lon}) h = fnv(fnv(h, s->data(), s->size()), "", 1);
    db->hash = h;
    return db;
}

uint32_t lookup(const pv_geodb &db, const uint8_t *addr, uint32_t addr_len)
{
    uint32_t w, words;
    if (addr_len == 4) { w = db.start4; words = 1; }
    else if (addr_len == 16 && db.ip_version == 6) { w = db.node_count ? 0 : PV_GEO_LEAF; words = 4; }
    else return 0; // an IPv6 address in an IPv4 tree: no entry
    for (uint32_t k = 0; k < words; k++) {
        const uint8_t *a = addr + 4 * k;
        w = pv_geo_step32(db.tree.data(), db.node_count, w, (uint32_t)a[0] << 24 | (uint32_t)a[1] << 16 | (uint32_t)a[2] << 8 | a[3]);
    }
    return pv_geo_id(w);
}

} // namespace pvgeo

// ====================================================================== C ABI
extern "C" {

const char *pv_geodb_last_error(void) { return g_err.c_str(); }

int pv_geodb_open(const uint8_t *bytes, size_t len, uint32_t kind, pv_geodb **db)
{
    if (!db) { g_err = "bad argument"; return PV_EINVAL; }
    *db = pvgeo::open(bytes, len, kind, g_err);
    return *db ? PV_OK : PV_EINVAL;
}

int pv_geodb_open_file(const char *path, uint32_t kind, pv_geodb **db)
{
    if (!path || !db) { g_err = "bad argument"; return PV_EINVAL; }
    *db = nullptr;
    FILE *f = fopen(path, "rb");
    if (!f) { g_err = std::string("cannot open ") + path; return PV_EINVAL; }
    std::vector<uint8_t> buf;
    uint8_t chunk[65536];
    size_t n;
    while ((n = fread(chunk, 1, sizeof chunk, f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
    fclose(f);
    return pv_geodb_open(buf.data(), buf.size(), kind, db);
}

void pv_geodb_close(pv_geodb *db) { delete db; }

uint32_t pv_geodb_entries(const pv_geodb *db) { return db ? (uint32_t)db->dict.size() : 0; }

uint64_t pv_geodb_hash(const pv_geodb *db) { return db ? db->hash : 0; }

int pv_geodb_entry(const pv_geodb *db, uint32_t id, const char **name, const char **lat, const char **lon)
{
    if (!db || id >= db->dict.size()) { g_err = "no such dictionary id"; return PV_EINVAL; }
    if (name) *name = db->dict[id].name.c_str();
    if (lat) *lat = db->dict[id].lat.c_str();
    if (lon) *lon = db->dict[id].lon.c_str();
    return PV_OK;
}

int pv_geodb_lookup(const pv_geodb *db, const uint8_t *addrs, size_t n, uint32_t addr_len, uint32_t *ids)
{
    if (!db || (n && (!addrs || !ids)) || (addr_len != 4 && addr_len != 16)) { g_err = "bad argument"; return PV_EINVAL; }
    for (size_t i = 0; i < n; i++) ids[i] = pvgeo::lookup(*db, addrs + i * addr_len, addr_len);
    return PV_OK;
}

} // extern "C"
