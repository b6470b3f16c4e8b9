"""Hand-built NetFlow v1 / v5 / v7 datagrams as classic-pcap records (test infrastructure): the
export headers and flow records of 3rd/netflow/netflow.h, over the link / IP / UDP builders of
tests/dhcp_cases.py, and the seeded mutations of the reference's nf5.pcap fixture."""
import struct

import numpy as np

from tests import dhcp_cases as dc

T0 = dc.T0
PORT = 2055
HDR = {1: 16, 5: 24, 7: 24}
REC = {1: 48, 5: 48, 7: 52}
MAXFLOWS = {1: 24, 5: 30, 7: 30}


def flow(src="192.168.1.1", dst="192.168.1.2", if_in=1, if_out=2, packets=1, octets=100, sport=1000, dport=80, proto=6, tos=0):
    return dict(src=src, dst=dst, if_in=if_in, if_out=if_out, packets=packets, octets=octets, sport=sport, dport=dport,
                proto=proto, tos=tos)


def wire_record(version: int, f: dict) -> bytes:
    head = dc.ip4(f["src"]) + dc.ip4(f["dst"]) + dc.ip4("10.9.9.9") + struct.pack(
        ">HHIIIIHH", f["if_in"], f["if_out"], f["packets"], f["octets"], 1000, 2000, f["sport"], f["dport"])
    if version == 1:
        # pad1(2) protocol tos tcp_flags pad(3) reserved(4)
        return head + struct.pack(">HBBB3sI", 0, f["proto"], f["tos"], 0x10, b"", 0)
    tail = struct.pack(">BBBBHHBBH", 0, 0x10, f["proto"], f["tos"], 64500, 64501, 24, 24, 0)
    return head + tail + (struct.pack(">I", 0x0a000001) if version == 7 else b"")


def datagram(version: int, flows, time=(T0, 5000), count=None, cut: int = 0, extra: bytes = b"") -> bytes:
    """the UDP payload: header (count: the header's count field, by default len(flows)), the flow
    records, minus `cut` trailing bytes, plus `extra`"""
    n = len(flows) if count is None else count
    h = struct.pack(">HHIII", version, n, 123456, time[0], time[1])
    if version in (5, 7):
        h += struct.pack(">II", 77, 0)
    body = h + b"".join(wire_record(version, f) for f in flows)
    return body[:len(body) - cut] + extra


def packet(payload: bytes, sec=T0, frac=0, dp=PORT, sp=50000, src="10.0.0.2", dst="10.0.0.3", vlan=None, v6=False, ihl=5,
           caplen=None) -> bytes:
    """one Ethernet record carrying the payload over UDP"""
    if v6:
        frame = dc.eth(dc.ipv6(dc.udp(payload, sp, dp), src=bytes.fromhex("20010db8000000000000000000000002")), 0x86DD, vlan=vlan)
    else:
        frame = dc.eth(dc.ipv4(dc.udp(payload, sp, dp), src=src, dst=dst, ihl=ihl), vlan=vlan)
    return dc.record(frame, sec, frac, caplen)


def flows_n(n: int, base: int = 0):
    """n flows, number base on, of one endless sequence: addresses and ports repeat every 24 flows
    (so a sketch never holds more than 24 distinct values, whatever the case takes), interfaces,
    protocols, tos values, packets and octets on their own cycles. tests/test_flow_host.py feeds
    the sequence's values to the reference's sketch: its rounded estimates are the distinct counts."""
    out = []
    for i in range(base, base + n):
        k = i % 24
        out.append(flow(src="172.16.0.%d" % (1 + k % 7), dst="172.16.1.%d" % (1 + k % 9), if_in=i % 3, if_out=3 + i % 2,
                        packets=1 + i % 5, octets=40 + 13 * (i % 17), sport=1024 + k % 11, dport=(22, 53, 80, 443, 6000)[k % 5],
                        proto=(6, 17, 1)[i % 3], tos=(0, 0xb8, 0xc0, 0x2b)[i % 4]))
    return out


def zero_flows():
    """port 0 and address 0.0.0.0 records, zero weights, and every field at its maximum"""
    return [flow(src="0.0.0.0"), flow(dst="0.0.0.0"), flow(sport=0), flow(dport=0),
            flow(sport=0, dport=0, src="0.0.0.0", dst="0.0.0.0"), flow(packets=0), flow(octets=0),
            flow(if_in=65535, if_out=65535, sport=65535, dport=65535, proto=255, tos=255, packets=0xFFFFFFFF, octets=0xFFFFFFFF)]


def filler(sec=T0, frac=0) -> bytes:
    """a 64-byte UDP packet that is no flow datagram (port 53 to 40000)"""
    return dc.filler(sec, frac)


def fixture_mutations(recs: bytes, n: int, seed: int = 11):
    """n variants of a capture's records: byte flips in the NetFlow header (version, count, times) of
    a record, truncations of the captured bytes, and UDP / IP lengths one short and one over"""
    rng = np.random.default_rng(seed)
    rs, pos = [], 0
    while pos + 16 <= len(recs):
        cap = struct.unpack_from("<I", recs, pos + 8)[0]
        rs.append(bytearray(recs[pos:pos + 16 + cap]))
        pos += 16 + cap
    out = []
    for i in range(n):
        cur = [bytearray(r) for r in rs]
        r = cur[int(rng.integers(0, len(cur)))]
        kind = i % 4
        if kind == 0:  # a flip in the NetFlow header: record byte 16 + 42 + [0, 16)
            r[58 + int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:  # version / count bytes replaced
            r[58 + int(rng.integers(0, 4))] = int(rng.integers(0, 32))
        elif kind == 2:  # truncation of the captured bytes
            cap = int(rng.integers(0, len(r) - 16))
            del r[16 + cap:]
            struct.pack_into("<I", r, 8, cap)
        else:  # IP total length and UDP length one short / one over
            d = 1 if rng.integers(0, 2) else -1
            struct.pack_into(">H", r, 16 + 16, struct.unpack_from(">H", r, 16 + 16)[0] + d)
            struct.pack_into(">H", r, 16 + 38, struct.unpack_from(">H", r, 16 + 38)[0] + d)
        out.append(b"".join(bytes(x) for x in cur))
    return out
