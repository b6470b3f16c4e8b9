"""Test helper (not a conftest): an independent pure-Python MaxMind DB 2.0 reader written from the
format specification, the two string renderings of the reference's GeoDB.cpp restated
(_getGeoLoc :179-244, _getASNString :371-413), and a tiny MMDB writer for synthetic trees."""
import ipaddress
import struct

MARKER = b"\xab\xcd\xefMaxMind.com"


class Ptr(int):
    """a decoded pointer (kept apart from integers)"""


class Reader:
    def __init__(self, data: bytes):
        self.buf = data
        m = data.rfind(MARKER)
        assert m >= 0
        self.meta, _ = self._decode(m + len(MARKER), m + len(MARKER))
        self.node_count = self.meta["node_count"][2]  # integers decode as (sign, type, value)
        self.record_size = self.meta["record_size"][2]
        self.ip_version = self.meta["ip_version"][2]
        self.tree_bytes = self.node_count * self.record_size // 4
        self.data_base = self.tree_bytes + 16

    # ---- data section
    def _decode(self, off, base):
        c = self.buf[off]
        off += 1
        t = c >> 5
        if t == 1:
            ss = (c >> 3) & 3
            raw = self.buf[off:off + ss + 1]
            off += ss + 1
            v = int.from_bytes(raw, "big")
            if ss < 3:
                v |= (c & 7) << (8 * (ss + 1))
            v += (0, 2048, 526336, 0)[ss]
            return Ptr(v), off
        if t == 0:
            t = 7 + self.buf[off]
            off += 1
        size = c & 31
        if size == 29:
            size = 29 + self.buf[off]
            off += 1
        elif size == 30:
            size = 285 + int.from_bytes(self.buf[off:off + 2], "big")
            off += 2
        elif size == 31:
            size = 65821 + int.from_bytes(self.buf[off:off + 3], "big")
            off += 3
        if t == 7:
            out = {}
            for _ in range(size):
                k, off = self._decode(off, base)
                if isinstance(k, Ptr):
                    k = self._decode(base + k, base)[0]
                v, off = self._decode(off, base)
                if isinstance(v, Ptr):
                    v = self._decode(base + v, base)[0]
                out[k] = v
            return out, off
        if t == 11:
            out = []
            for _ in range(size):
                v, off = self._decode(off, base)
                if isinstance(v, Ptr):
                    v = self._decode(base + v, base)[0]
                out.append(v)
            return out, off
        if t == 14:
            return bool(size), off
        raw = self.buf[off:off + size]
        off += size
        if t == 2:
            return raw.decode("utf-8"), off
        if t == 3:
            return struct.unpack(">d", raw)[0], off
        if t == 4:
            return bytes(raw), off
        if t in (5, 6, 9, 10):
            return ("u", t, int.from_bytes(raw, "big")), off
        if t == 8:
            v = int.from_bytes(raw, "big")
            if size == 4 and v >= 1 << 31:
                v -= 1 << 32
            return ("i", t, v), off
        if t == 15:
            return ("f", struct.unpack(">f", raw)[0]), off
        raise ValueError(f"type {t}")

    def data_at(self, doff):
        v = self._decode(self.data_base + doff, self.data_base)[0]
        if isinstance(v, Ptr):
            v = self._decode(self.data_base + v, self.data_base)[0]
        return v

    # ---- search tree
    def record(self, node, side):
        rs = self.record_size
        b = self.buf[node * rs // 4:(node + 1) * rs // 4]
        if rs == 24:
            return int.from_bytes(b[3 * side:3 * side + 3], "big")
        if rs == 28:
            if side == 0:
                return ((b[3] & 0xF0) << 20) | int.from_bytes(b[0:3], "big")
            return ((b[3] & 0x0F) << 24) | int.from_bytes(b[4:7], "big")
        return int.from_bytes(b[4 * side:4 * side + 4], "big")

    def find(self, addr: bytes):
        """the data offset of a packed address, or None (no entry)"""
        nc = self.node_count
        node = 0
        if len(addr) == 16 and self.ip_version == 4:
            return None
        if nc == 0:
            return None
        if len(addr) == 4 and self.ip_version == 6:
            for _ in range(96):
                if node >= nc:
                    break
                node = self.record(node, 0)
        for i in range(len(addr) * 8):
            if node >= nc:
                break
            node = self.record(node, (addr[i >> 3] >> (7 - (i & 7))) & 1)
        if node <= nc:  # a node after the last bit, or the "no data" record
            return None
        return node - nc - 16

    def leaves(self):
        """(prefix bits as int, prefix length, record) of every record the root reaches that is not a node"""
        if self.node_count == 0:
            return
        stack = [(0, 0, 0)]
        seen = set()
        while stack:
            node, bits, depth = stack.pop()
            for side in (0, 1):
                r = self.record(node, side)
                nb, nd = (bits << 1) | side, depth + 1
                if r < self.node_count:
                    if (r, nd) not in seen and nd < 128:
                        seen.add((r, nd))
                        stack.append((r, nb, nd))
                else:
                    yield nb, nd, r


def render_city(rec):
    """(location, latitude, longitude) of a decoded City record: _getGeoLoc"""
    def get(*path):
        cur = rec
        for k in path:
            if isinstance(k, int):
                if not isinstance(cur, list) or k >= len(cur):
                    return None
                cur = cur[k]
            else:
                if not isinstance(cur, dict) or k not in cur:
                    return None
                cur = cur[k]
        return cur
    loc = ""
    v = get("continent", "code")
    if isinstance(v, str):
        loc += v
    v = get("country", "names", "en")
    if v is None:
        v = get("country", "iso_code")
    if isinstance(v, str):
        loc += "/" + v
    v = get("subdivisions", 0, "iso_code")
    if isinstance(v, str):
        loc += "/" + v
    v = get("city", "names", "en")
    if isinstance(v, str):
        loc += "/" + v
    lat = get("location", "latitude")
    lon = get("location", "longitude")
    return (loc, "%f" % lat if isinstance(lat, float) else "", "%f" % lon if isinstance(lon, float) else "")


def render_asn(rec):
    """the ASN string of a decoded ISP / ASN record: _getASNString"""
    s = ""
    v = rec.get("autonomous_system_number") if isinstance(rec, dict) else None
    if isinstance(v, tuple) and v[0] in ("u", "i") and v[1] in (5, 6, 8, 9):
        s += str(v[2])
    elif isinstance(v, str):
        s += v
    v = rec.get("autonomous_system_organization") if isinstance(rec, dict) else None
    if isinstance(v, str):
        s += "/" + v
    return s


def lookup(reader: Reader, kind: str, addr: bytes):
    """(name, lat, lon) as the reference's getGeoLoc / getASNString give it"""
    off = reader.find(addr)
    if off is None:
        return ("Unknown", "", "")
    rec = reader.data_at(off)
    return render_city(rec) if kind == "city" else (render_asn(rec), "", "")


# ---------------------------------------------------------------- writer
def _ctrl(t, size):
    assert size < 29 + 256
    if t <= 7:
        head = [t << 5]
    else:
        head = [0, t - 7]
    if size < 29:
        head[0] |= size
        return bytes(head)
    head[0] |= 29
    return bytes(head) + bytes([size - 29])


class U16(int):
    pass


class U32(int):
    pass


class U64(int):
    pass


class I32(int):
    pass


class RawPtr(int):
    """a pointer to this data-section offset (32-bit form)"""


def enc(v):
    if isinstance(v, RawPtr):
        return bytes([(1 << 5) | (3 << 3)]) + int(v).to_bytes(4, "big")
    if isinstance(v, bool):
        return _ctrl(14, int(v))
    if isinstance(v, str):
        b = v.encode()
        return _ctrl(2, len(b)) + b
    if isinstance(v, float):
        return _ctrl(3, 8) + struct.pack(">d", v)
    if isinstance(v, dict):
        out = _ctrl(7, len(v))
        for k, x in v.items():
            out += enc(k) + enc(x)
        return out
    if isinstance(v, list):
        return _ctrl(11, len(v)) + b"".join(enc(x) for x in v)
    if isinstance(v, I32):
        return _ctrl(8, 4) + (int(v) & 0xFFFFFFFF).to_bytes(4, "big")
    if isinstance(v, U16):
        return _ctrl(5, 2) + int(v).to_bytes(2, "big")
    if isinstance(v, U64):
        return _ctrl(9, 8) + int(v).to_bytes(8, "big")
    if isinstance(v, int):
        return _ctrl(6, 4) + int(v).to_bytes(4, "big")
    raise TypeError(type(v))


def write_mmdb(prefixes, record_size=24, ip_version=6, raw_data=None, meta_override=None, extra_data=b""):
    """prefixes: [(cidr string, record dict)] (an IPv4 cidr in an ip_version 6 tree lands under ::/96).
    raw_data: {cidr: bytes} entries written as they are (for malformed records). Returns the file bytes."""
    # binary trie: node = [left, right]; a child is None (no data), a list (node) or ("d", index)
    root = [None, None]
    datas = []

    def data_index(rec):
        datas.append(rec)
        return len(datas) - 1

    items = [(c, ("rec", r)) for c, r in prefixes] + [(c, ("raw", b)) for c, b in (raw_data or {}).items()]
    for cidr, payload in items:
        net = ipaddress.ip_network(cidr)
        bits, plen = int(net.network_address), net.prefixlen
        width = 32 if net.version == 4 else 128
        if net.version == 4 and ip_version == 6:
            plen, width = plen + 96, 128
        assert plen >= 1
        node = root
        for i in range(plen):
            b = (bits >> (width - 1 - i)) & 1
            if i == plen - 1:
                node[b] = ("d", data_index(payload))
            else:
                if not isinstance(node[b], list):
                    node[b] = [None, None]
                node = node[b]
    # number the nodes breadth first
    nodes, order = [root], {id(root): 0}
    for n in nodes:
        for ch in n:
            if isinstance(ch, list):
                order[id(ch)] = len(nodes)
                nodes.append(ch)
    nc = len(nodes)
    blob, offs = b"", []
    for kind, d in datas:
        offs.append(len(blob))
        blob += enc(d) if kind == "rec" else d
    blob += extra_data

    def recval(ch):
        if ch is None:
            return nc
        if isinstance(ch, list):
            return order[id(ch)]
        return nc + 16 + offs[ch[1]]

    tree = b""
    for n in nodes:
        l, r = recval(n[0]), recval(n[1])
        if record_size == 24:
            tree += l.to_bytes(3, "big") + r.to_bytes(3, "big")
        elif record_size == 28:
            tree += (l & 0xFFFFFF).to_bytes(3, "big") + bytes([((l >> 24) << 4) | (r >> 24)]) + (r & 0xFFFFFF).to_bytes(3, "big")
        else:
            tree += l.to_bytes(4, "big") + r.to_bytes(4, "big")
    meta = {"node_count": nc, "record_size": U16(record_size), "ip_version": U16(ip_version),
            "database_type": "Test", "binary_format_major_version": U16(2), "binary_format_minor_version": U16(0)}
    meta.update(meta_override or {})
    return tree + b"\0" * 16 + blob + MARKER + enc(meta)
