"""Hand-built DNS queries with EDNS Client Subnet options as classic-pcap records, and the model of
the DNS v1 handler's top_geoLoc_ecs / top_asn_ecs (test infrastructure, no GPU): the link, IP and
UDP builders of tests/dhcp_cases.py and the TCP header of tests/bgp_cases.py.

The model applies the reference's address rule (libs/visor_dns/DnsAdditionalRecord.h:80-98:
client_subnet as a full address) in Python: IPv4 the first four option address bytes, IPv6 only the
first eight, missing bytes zero; then looks the address up with the independent reader of
tests/mmdb_ref.py (a lookup that finds nothing is "Unknown")."""
import ipaddress
import struct

from tests import mmdb_ref as R
from tests.bgp_cases import ACK, PSH, SYN, tcp
from tests.dhcp_cases import T0, eth, ipv4, ipv6, record, udp

HOST = "192.168.0.0/24,fd00:aaaa::/64"
CLIENT4, RESOLVER4 = "192.168.0.7", "10.9.8.7"
CLIENT6 = ipaddress.ip_address("fd00:aaaa::5").packed
RESOLVER6 = ipaddress.ip_address("2001:db8:53::1").packed


def v4(s, n=4, extra=b""):
    """(family 1, the first n bytes of the dotted address + extra)"""
    return (1, ipaddress.ip_address(s).packed[:n] + extra)


def v6(s, n=16, tail=None):
    """(family 2, the first n bytes of the address; tail replaces bytes 8..16)"""
    raw = ipaddress.ip_address(s).packed
    if tail is not None:
        raw = raw[:8] + tail
    return (2, raw[:n])


# the known addresses of tests/golden/kat_geo.json and some neither database holds; subnet i is
# carried by 3 * 2^i queries, so the per-key counts are distinct and the order of a top is defined
SUBNETS = [
    v4("89.160.20.112"),                                     # EU/Sweden/E/Linköping
    v4("1.128.0.0", 3),                                      # three bytes: 1.128.0.0, 1221/Telstra Pty Ltd
    v4("81.2.69.142", 4, b"\xde\xad"),                       # six bytes: the last two are ignored
    v4("8.8.8.8"),                                           # city Unknown, ASN ""
    v4("12.81.92.0"),                                        # ASN "7018"
    v4("216.160.83.56"),                                     # NA/United States/WA/Milton, ASN "209"
    v6("2a02:dac0::", 8),                                    # exactly eight bytes: EU/Russia
    v6("2001:218::", 4),                                     # fewer than eight: AS/Japan
    v6("2001:1700::", 16, bytes.fromhex("deadbeef00c0ffee")),  # the last eight do not matter: 6730/Sunrise ...
    v6("2001:db8::77", 16),                                  # 2001:db8:: after the cut, in neither
]


def ecs_option(family, addr, source=None, code=8):
    source = 8 * len(addr) if source is None else source
    data = struct.pack(">HBB", family, source, 0) + addr
    return struct.pack(">HH", code, len(data)) + data


def opt_rr(options=b""):
    """the OPT pseudo-record: root name, type 41, UDP size 4096, no flags"""
    return b"\x00" + struct.pack(">HHIH", 41, 4096, 0, len(options)) + options


def message(txid, name, additional=b"", qr=0, arcount=None, answers=b"", ancount=0):
    q = b"".join(bytes([len(l)]) + l.encode() for l in name.split(".")) + b"\x00" + struct.pack(">HH", 1, 1)
    ar = (1 if additional else 0) if arcount is None else arcount
    flags = 0x8180 if qr else 0x0100
    return struct.pack(">HHHHHH", txid, flags, 1, ancount, 0, ar) + q + answers + additional


def udp_frame(msg, n=0, six=False, to_resolver=True):
    """Ethernet / IPv4 or IPv6 / UDP, client port 20000 + n % 40000, resolver port 53"""
    sp, dp = (20000 + n % 40000, 53) if to_resolver else (53, 20000 + n % 40000)
    if six:
        a, b = (CLIENT6, RESOLVER6) if to_resolver else (RESOLVER6, CLIENT6)
        return eth(ipv6(udp(msg, sp, dp), 17, a, b), 0x86DD)
    a, b = (CLIENT4, RESOLVER4) if to_resolver else (RESOLVER4, CLIENT4)
    return eth(ipv4(udp(msg, sp, dp), 17, a, b))


def tcp_query(msg, port=41000, seq=7000):
    """a minimal flow to port 53: SYN, then one in-order segment with the 2-byte length prefix"""
    syn = eth(ipv4(tcp(b"", port, 53, seq, SYN), 6, CLIENT4, RESOLVER4))
    seg = eth(ipv4(tcp(struct.pack(">H", len(msg)) + msg, port, 53, seq + 1, PSH | ACK), 6, CLIENT4, RESOLVER4))
    return syn, seg


def ecs_query(n, sub, six=False):
    """the frame of query n (qname q<n % 7>.example.com) carrying subnet (family, address bytes)"""
    return udp_frame(message(n & 0xffff, f"q{n % 7}.example.com", opt_rr(ecs_option(*sub))), n, six)


def stamps(t0=T0, step_us=20):
    us = 0
    while True:
        yield t0 + us // 1000000, us % 1000000
        us += step_us


def packets(t0=T0, step_us=20, extras=True, tcp_flow=True, subnets=SUBNETS, scale=1, tcp_port=41000):
    """[(sec, usec, frame, what)]: what = the (family, address bytes) of a counted ECS query, "event" for
    a DNS event counted in neither top, None for a packet that is no DNS event. Subnet i rides on
    3 * 2^i * scale queries, interleaved round by round (so the first rounds hold every subnet); every
    third query travels over IPv6. extras: the cases that must be counted nowhere; tcp_flow: one more
    query of the last subnet over TCP (a flow of its own from tcp_port), which is counted."""
    seq = []
    for i, sub in enumerate(subnets):
        seq += [(k, i) for k in range(3 * (1 << i) * scale)]
    seq.sort()
    out = []
    ts = stamps(t0, step_us)
    for n, (_, i) in enumerate(seq):
        out.append((*next(ts), ecs_query(n, subnets[i], six=n % 3 == 2), subnets[i]))
    if extras:
        sub = subnets[0]
        other = [
            message(1, "fam3.example.com", opt_rr(ecs_option(3, sub[1]))),                       # a family-3 option
            message(2, "resp.example.com", opt_rr(ecs_option(*sub)), qr=1),                      # a response carrying ECS
            message(3, "noar.example.com"),                                                      # ARCOUNT = 0
            message(4, "nocs.example.com", opt_rr(struct.pack(">HH", 10, 8) + bytes(8))),         # OPT, a COOKIE, no CSUBNET
            message(5, "bare.example.com", opt_rr()),                                            # OPT without options
        ]
        for k, m in enumerate(other):
            out.insert(7 + 11 * k, (0, 0, udp_frame(m, 50000 + k, to_resolver=not (k == 1)), "event"))
    if tcp_flow:
        syn, seg = tcp_query(message(77, "tcp.example.com", opt_rr(ecs_option(*subnets[-1]))), tcp_port)
        out.insert(len(out) // 2, (0, 0, syn, None))
        out.insert(len(out) // 2 + 5, (0, 0, seg, subnets[-1]))
    # (stamps in capture order, whatever was inserted)
    ts = stamps(t0, step_us)
    return [(*next(ts), fr, what) for _, _, fr, what in out]


def records(pk) -> bytes:
    return b"".join(record(fr, s, u) for s, u, fr, _ in pk)


def pcap_of(pk) -> bytes:
    return struct.pack("<IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, 65535, 1) + records(pk)


def readers(city_path, asn_path):
    return {"city": R.Reader(open(city_path, "rb").read()), "asn": R.Reader(open(asn_path, "rb").read())}


def counted(pk):
    """the (family, address bytes) of the counted ECS queries, in capture order"""
    return [w for _, _, _, w in pk if isinstance(w, tuple)]


def full_address(sub) -> bytes:
    """the reference's client_subnet as a full address: 4 or 16 bytes, network order"""
    fam, addr = sub
    if fam == 1:
        return (addr + bytes(4))[:4]
    return (addr[:8] + bytes(8))[:8] + bytes(8)


def subnet_text(sub) -> str:
    """the top_query_ecs name of a subnet: inet_ntop of the kept bytes"""
    return str(ipaddress.ip_address(full_address(sub)))


def lookup(rd, kind, sub):
    """(name, lat, lon) of a subnet in one database"""
    return R.lookup(rd[kind], kind, full_address(sub))


def expected(pk, rd, kinds=("city", "asn"), distinct=True):
    """{'top_geoLoc_ecs': [...], 'top_asn_ecs': [...]} as the JSON lists them (estimate descending,
    ties by name); distinct: assert that no two keys of a top share a count"""
    out = {"top_geoLoc_ecs": [], "top_asn_ecs": []}
    for kind in kinds:
        cnt = {}
        for sub in counted(pk):
            key = lookup(rd, kind, sub)
            cnt[key] = cnt.get(key, 0) + 1
        items = []
        for (name, lat, lon), n in cnt.items():
            it = {"name": name, "estimate": n}
            if kind == "city" and lat and lon:
                it["lat"], it["lon"] = lat, lon
            items.append(it)
        items.sort(key=lambda it: (-it["estimate"], it["name"]))
        if distinct:
            assert len({it["estimate"] for it in items}) == len(items), "per-key counts must be distinct"
        out["top_geoLoc_ecs" if kind == "city" else "top_asn_ecs"] = items
    return out


def expected_query_ecs(pk):
    """top_query_ecs of the counted queries: [{name, estimate}], estimate descending, ties by name"""
    cnt = {}
    for sub in counted(pk):
        cnt[subnet_text(sub)] = cnt.get(subnet_text(sub), 0) + 1
    return sorted(({"name": k, "estimate": v} for k, v in cnt.items()), key=lambda it: (-it["estimate"], it["name"]))


def passes(rd, what, geoloc_notfound=False, asn_notfound=False, city=True, asn=True):
    """DnsStreamHandler::_filtering's last two checks for one packet of packets(): an ECS query
    whose lookup equals "Unknown" in every family that is on (a family without its database passes
    nothing)"""
    if not isinstance(what, tuple):
        return False
    if geoloc_notfound and (not city or lookup(rd, "city", what)[0] != "Unknown"):
        return False
    if asn_notfound and (not asn or lookup(rd, "asn", what)[0] != "Unknown"):
        return False
    return True


# ---------------------------------------------------------------- reading a capture back
def pcap_frames(blob: bytes):
    """the frames of a classic little-endian pcap"""
    assert struct.unpack_from("<I", blob)[0] in (0xA1B2C3D4, 0xA1B23C4D)
    pos = 24
    while pos + 16 <= len(blob):
        cap = struct.unpack_from("<I", blob, pos + 8)[0]
        yield blob[pos + 16:pos + 16 + cap]
        pos += 16 + cap


def udp_dns_message(fr: bytes):
    """the payload of an Ethernet / IPv4 or IPv6 / UDP frame with port 53 on either side, else None"""
    et = struct.unpack_from(">H", fr, 12)[0]
    if et == 0x0800 and fr[23] == 17:
        l4 = 14 + 4 * (fr[14] & 15)
    elif et == 0x86DD and fr[20] == 17:
        l4 = 54
    else:
        return None
    sp, dp = struct.unpack_from(">HH", fr, l4)
    return fr[l4 + 8:] if 53 in (sp, dp) else None


def _skip_name(m, off):
    while off < len(m):
        n = m[off]
        if n == 0:
            return off + 1
        if n & 0xC0:
            return off + 2
        off += 1 + n
    return off


def ecs_of_message(m: bytes):
    """(family, address bytes) of a query whose first additional record is an OPT record opening
    with a CSUBNET option of family 1 / 2 and at least one address byte, else None"""
    if len(m) < 12:
        return None
    flags, qd, an, ns, ar = struct.unpack_from(">HHHHH", m, 2)
    if flags & 0x8000 or not ar:
        return None
    off = 12
    for _ in range(qd):
        off = _skip_name(m, off) + 4
    for _ in range(an + ns):
        off = _skip_name(m, off)
        if off + 10 > len(m):
            return None
        off += 10 + struct.unpack_from(">H", m, off + 8)[0]
    off = _skip_name(m, off)
    if off + 10 > len(m):
        return None
    rtype, dlen = struct.unpack_from(">H", m, off)[0], struct.unpack_from(">H", m, off + 8)[0]
    data = m[off + 10:off + 10 + dlen]
    if rtype != 41 or len(data) < 9 or len(data) != dlen or struct.unpack_from(">H", data)[0] != 8:
        return None
    family = struct.unpack_from(">H", data, 4)[0]
    if family not in (1, 2):
        return None
    olen = struct.unpack_from(">H", data, 2)[0]
    return (family, data[8:4 + olen][:16])
