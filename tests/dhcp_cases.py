"""Hand-built DHCP / DHCPv6 packets as classic-pcap records (test infrastructure; scapy and dpkt are
not installed): link, IP and UDP layers, BOOTP messages with options, request/ack streams, and the
random and adversarial payload corpus of the decoder fuzz."""
import struct

import numpy as np

MAC_C = bytes.fromhex("784f437819bc")
MAC_S = bytes.fromhex("b827eb0cb3e2")
T0 = 1700000000


def ip4(s):
    return bytes(int(x) for x in s.split("."))


def record(frame: bytes, sec: int = T0, frac: int = 0, caplen=None) -> bytes:
    cap = len(frame) if caplen is None else min(caplen, len(frame))
    return struct.pack("<IIII", sec, frac, cap, len(frame)) + frame[:cap]


def eth(payload: bytes, etype: int = 0x0800, src: bytes = MAC_C, dst: bytes = b"\xff" * 6, vlan=None) -> bytes:
    tag = b"" if vlan is None else struct.pack(">HH", 0x8100, vlan)
    return dst + src + tag + struct.pack(">H", etype) + payload


def ipv4(payload: bytes, proto: int = 17, src="0.0.0.0", dst="255.255.255.255", ihl: int = 5, frag: int = 0, total=None) -> bytes:
    hl = ihl * 4
    tot = hl + len(payload) if total is None else total
    h = struct.pack(">BBHHHBBH4s4s", 0x40 | ihl, 0, tot, 1, frag, 64, proto, 0, ip4(src), ip4(dst))
    return h + bytes(hl - 20) + payload


def ipv6(payload: bytes, nxt: int = 17, src=None, dst=None, hop_by_hop: bool = False) -> bytes:
    src = src or bytes.fromhex("fe800000000000000a0027fffed410bb")
    dst = dst or bytes.fromhex("ff020000000000000000000000010002")
    ext = b""
    if hop_by_hop:
        ext = bytes([nxt, 0]) + bytes(6)  # next header, length 0 (8 bytes), PadN
        nxt = 0
    return struct.pack(">IHBB", 0x60000000, len(ext) + len(payload), nxt, 64) + src + dst + ext + payload


def udp(payload: bytes, sp: int, dp: int) -> bytes:
    return struct.pack(">HHHH", sp, dp, 8 + len(payload), 0) + payload


def options(opts) -> bytes:
    """[(type, value bytes)] -> TLVs; type 0 / 255 entries are the one-byte PAD / END"""
    out = b""
    for t, v in opts:
        out += bytes([t]) if t in (0, 255) else bytes([t, len(v)]) + v
    return out


def bootp(mtype=None, xid: int = 1, yiaddr="0.0.0.0", chaddr: bytes = MAC_C, opts=(), op: int = 1, htype: int = 1,
          hlen: int = 6, end: bool = True) -> bytes:
    h = struct.pack(">BBBBIHH4s4s4s4s16s64s128sI", op, htype, hlen, 0, xid, 0, 0, ip4("0.0.0.0"), ip4(yiaddr), ip4("0.0.0.0"),
                    ip4("0.0.0.0"), chaddr.ljust(16, b"\0"), b"", b"", 0x63825363)
    o = list(opts)
    if mtype is not None:
        o = [(53, bytes([mtype]))] + o
    return h + options(o) + (b"\xff" if end else b"")


def dhcp4(mtype, xid=1, sec=T0, frac=0, src_mac=MAC_C, sp=68, dp=67, **kw) -> bytes:
    """one Ethernet / IPv4 / UDP record"""
    return record(eth(ipv4(udp(bootp(mtype, xid, **kw), sp, dp)), src=src_mac), sec, frac)


def dhcp6_msg(mtype: int, opts=()) -> bytes:
    out = bytes([mtype, 0, 0, 1])
    for t, v in opts:
        out += struct.pack(">HH", t, len(v)) + v
    return out


def dhcp6(mtype, opts=(), sec=T0, frac=0, src_mac=MAC_S, sp=547, dp=546, **kw) -> bytes:
    return record(eth(ipv6(udp(dhcp6_msg(mtype, opts), sp, dp), **kw), 0x86DD, src=src_mac), sec, frac)


def filler(sec=T0, frac=0, size: int = 64) -> bytes:
    """a 64-byte non-DHCP UDP packet (port 53 to 40000)"""
    pay = bytes(size - 14 - 20 - 8)
    return record(eth(ipv4(udp(pay, 53, 40000), src="10.0.0.1", dst="10.0.0.2")), sec, frac)


def request(xid, host=b"host", sec=T0, frac=0, mac=MAC_C):
    return dhcp4(3, xid, sec, frac, src_mac=mac, chaddr=mac, opts=[] if host is None else [(12, host)])


def ack(xid, yiaddr="192.168.2.205", sec=T0, frac=0, server="192.168.2.1"):
    return dhcp4(5, xid, sec, frac, src_mac=MAC_S, sp=67, dp=68, op=2, yiaddr=yiaddr, opts=[(54, ip4(server))])


def offer(xid, yiaddr="192.168.2.205", sec=T0, frac=0, server="192.168.2.1"):
    return dhcp4(2, xid, sec, frac, src_mac=MAC_S, sp=67, dp=68, op=2, yiaddr=yiaddr, opts=[(54, ip4(server))])


def pair_stream(n: int, sec0: int = T0, clients: int = 37, step_us: int = 1000) -> bytes:
    """n records alternating REQUEST / ACK of the same xid, over `clients` client names and addresses"""
    out, t = [], 0
    for i in range(n):
        k = (i // 2) % clients
        s, us = sec0 + t // 1000000, t % 1000000
        if i % 2 == 0:
            out.append(request(1000 + i // 2, b"client-%d" % k, s, us, mac=bytes([2, 0, 0, 0, 0, k])))
        else:
            out.append(ack(1000 + i // 2, "10.1.%d.%d" % (k // 200, k % 200 + 1), s, us))
        t += step_us
    return b"".join(out)


def fuzz_payloads(n: int, seed: int = 7):
    """n UDP payloads: random bytes, valid messages, and the adversarial shapes (lengths 0..600 with
    239 / 240 / 241, PAD and END before option 53, a record past the end, duplicate options, len 0
    and len 255, htype / hlen other than 1 / 6), for v4 and v6"""
    rng = np.random.default_rng(seed)
    out = []
    fixed = [0, 1, 3, 4, 7, 8, 239, 240, 241, 242, 243, 244, 495, 496, 497, 600]
    for i in range(n):
        kind = i % 8
        ln = fixed[(i // 8) % len(fixed)] if (i // 8) % 3 == 0 else int(rng.integers(0, 601))
        if kind == 0:
            p = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
        elif kind == 1:  # a header with random option bytes behind it
            p = (bootp(None, int(rng.integers(0, 1 << 32)), end=False) + rng.integers(0, 256, 360, dtype=np.uint8).tobytes())[:max(ln, 236)]
        elif kind in (2, 3, 4):
            opts = []
            for _ in range(int(rng.integers(0, 7))):
                t = int(rng.choice([0, 0, 255, 12, 12, 53, 53, 54, 54, 1, 3, 61, int(rng.integers(1, 255))]))
                l = int(rng.choice([0, 0, 1, 1, 3, 4, 4, 5, 255, int(rng.integers(0, 256))]))
                opts.append((t, rng.integers(0, 256, l, dtype=np.uint8).tobytes()))
            ht, hl = (1, 6) if rng.integers(0, 4) else (int(rng.integers(0, 8)), int(rng.integers(0, 17)))
            p = bootp(int(rng.integers(0, 9)) if rng.integers(0, 5) else None, int(rng.integers(0, 1 << 32)),
                      "10.0.0.%d" % int(rng.integers(0, 4)), rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), opts,
                      htype=ht, hlen=hl, end=bool(rng.integers(0, 2)))
            if kind == 3:  # a record that runs past the end
                p = p[:max(0, len(p) - int(rng.integers(1, 12)))]
            elif kind == 4:
                p = p + bytes([int(rng.choice([12, 53, 54])), int(rng.integers(1, 256))]) + b"ab"
        elif kind in (5, 6):
            opts = [(int(rng.choice([1, 2, 2, 3, 8, 25])), rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes())
                    for _ in range(int(rng.integers(0, 5)))]
            p = dhcp6_msg(int(rng.integers(0, 9)), opts)
            if kind == 6:
                p = p[:int(rng.integers(0, len(p) + 1))]
        else:
            # PAD and END ahead of option 53
            p = bootp(None, i, opts=[(0, b"")] * int(rng.integers(0, 4)) + [(255, b"")] * int(rng.integers(0, 2)) +
                      [(53, b"\x03"), (12, b"h" * int(rng.choice([0, 1, 255])))])
            p = p[:ln] if ln >= 236 and rng.integers(0, 2) else p
        out.append(p)
    return out


def fuzz_records(n: int, seed: int = 7) -> bytes:
    """the payload corpus as Ethernet records: v4 ports for the BOOTP shapes, v6 ports (over IPv6) for the DHCPv6 ones"""
    out = []
    for i, p in enumerate(fuzz_payloads(n, seed)):
        if i % 8 in (5, 6):
            out.append(record(eth(ipv6(udp(p, 546, 547)), 0x86DD, src=MAC_S), T0 + i // 1000, i % 1000))
        else:
            out.append(record(eth(ipv4(udp(p, 68, 67))), T0 + i // 1000, i % 1000))
    return b"".join(out)
