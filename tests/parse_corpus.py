"""Seeded generator of adversarial L2-L4 frames, built from layers so that every family exists both
intact and damaged. Shared by tests/test_parse_fuzz.py (CPU: parse_record against the oracle's
parse_packet) and tests/test_gpu_parse_paths.py (the same shapes through every Net-pass path).

A corpus is a list of groups (family, linktype, host_spec, frames): the link type and the host
subnets are per-run settings on both sides, so frames that share them travel together."""
import random
import socket
import struct

V4_POOL = ["10.1.2.3", "10.200.0.9", "172.16.5.5", "192.168.1.7", "192.168.1.8", "8.8.8.8", "0.0.0.0", "11.0.0.1",
           "11.128.0.1"]
V6_POOL = ["2001:db8::1", "2001:db8::", "2001:db8::2", "2101:db8::1", "2201:db8::1", "2081:db8::1", "a001:db8::1", "::"]

# 0, 1, 2, 3 and 5 IPv4 subnets with /0 and /32 (the third and later ones take match4's loop with
# v4_all; a /0 in the first two takes the mask-0 rule), IPv6 CIDRs 0, 1, 7, 8, 9, 127 and 128
HOST_SPECS = [
    "",
    "10.0.0.0/8",
    "0.0.0.0/0",
    "10.0.0.0/8,192.168.1.7/32",
    "192.168.1.7/32,0.0.0.0/0",
    "10.0.0.0/8,172.16.0.0/12,192.168.1.7/32",
    "10.0.0.0/8,172.16.0.0/12,192.168.1.7/32,0.0.0.0/0,11.0.0.0/9",
    "10.0.0.0/8,172.16.0.0/12,192.168.1.8/32,11.0.0.0/9,192.168.1.7/32",
    "2001:db8::1/0",
    "2001:db8::1/1",
    "2001:db8::1/7",
    "2001:db8::1/8",
    "2001:db8::1/9",
    "2001:db8::1/127",
    "2001:db8::1/128",
    "10.0.0.0/8,2001:db8::1/0,2001:db8::1/128",
    "192.168.1.0/24,2001:db8::/32",
]
DEFAULT_SPEC = "10.0.0.0/8,2001:db8::/32"
FIVE_V4_SPEC = HOST_SPECS[6]
RAW_LINKTYPES = (101, 12, 14, 228, 229)


def be16(v):
    return struct.pack(">H", v & 0xFFFF)


def rbytes(rng, n):
    return rng.randbytes(n)


# ---------------------------------------------------------------- L4
def fuzz_l4(rng, proto, tag):
    """a UDP or TCP layer of 0-40 bytes (shorter than the header included), TCP with and without SYN"""
    n = rng.choice((0, 7, 8, 9, 19, 20, 21, 40)) if rng.random() < 0.5 else rng.randrange(0, 41)
    b = bytearray(rbytes(rng, n))
    if proto == 6 and n > 13:
        b[13] = (b[13] & ~2) | (2 if rng.random() < 0.5 else 0)
    if proto == 17 and n >= 6:
        b[4:6] = be16(n)
    return bytes(b)


def dns_l4(rng, proto, tag):
    """UDP: a valid DNS query to port 53 whose name carries the family, so a wrong l4off or l4len
    shows in the DNS tables; TCP: a bare 20-byte header (port 53 would enter DNS-over-TCP
    reassembly, which is another test's subject), with and without SYN"""
    if proto == 17:
        labels = [b"%s%d" % (tag.encode(), rng.randrange(0, 4)), b"t"]
        name = b"".join(bytes([len(x)]) + x for x in labels) + b"\0"
        msg = struct.pack(">HHHHHH", rng.randrange(0, 65536), 0x0100, 1, 0, 0, 0) + name + struct.pack(">HH", 1, 1)
        return struct.pack(">HHHH", 1024 + rng.randrange(0, 4000), 53, 8 + len(msg), 0) + msg
    flags = 0x02 if rng.random() < 0.5 else 0x10
    return struct.pack(">HHIIBBHHH", 1024 + rng.randrange(0, 4000), 443, rng.getrandbits(32), 0, 5 << 4, flags, 8192, 0, 0)


# ---------------------------------------------------------------- L3
def v4hdr(rng, payload, proto, ihl=5, ver=4, total="exact", frag=0x4000, src=None, dst=None):
    """total: 'zero', 'below_hl', 'hl', 'below' (inside the payload), 'exact', 'beyond'"""
    hl = max(ihl, 5) * 4
    n = hl + len(payload)
    tl = {"zero": 0, "below_hl": rng.randrange(1, 20), "hl": ihl * 4, "exact": n, "beyond": n + rng.randrange(1, 40),
          "below": hl + (rng.randrange(0, len(payload)) if payload else 0)}[total]
    src = socket.inet_aton(src or rng.choice(V4_POOL))
    dst = socket.inet_aton(dst or rng.choice(V4_POOL))
    h = bytes([(ver << 4) | ihl, 0]) + be16(tl) + be16(rng.getrandbits(16)) + be16(frag) + bytes([64, proto]) + b"\0\0" + src + dst
    return h + rbytes(rng, hl - 20) + payload


def ext_size(t, lb):
    return 8 if t == 44 else ((lb + 2) * 4 if t == 51 else (lb + 1) * 8)


def v6hdr(rng, payload, nxt, chain=(), paylen="exact", src=None, dst=None, past=False):
    """chain: (type, length byte) of each extension header in order; past: the last header's length
    byte is 255 while only its declared bytes are present. paylen: 'zero', 'short', 'exact', 'long'"""
    body = b""
    types = [t for t, _ in chain] + [nxt]
    for i, (t, lb) in enumerate(chain):
        size = ext_size(t, lb)
        wire_lb = 255 if (past and i == len(chain) - 1) else lb
        body += bytes([types[i + 1], wire_lb]) + rbytes(rng, size - 2)
    n = len(body) + len(payload)
    pl = {"zero": 0, "short": rng.randrange(0, n) if n else 0, "exact": n, "long": n + rng.randrange(1, 40)}[paylen]
    src = socket.inet_pton(socket.AF_INET6, src or rng.choice(V6_POOL))
    dst = socket.inet_pton(socket.AF_INET6, dst or rng.choice(V6_POOL))
    return bytes([0x60, 0, 0, 0]) + be16(pl) + bytes([types[0], 64]) + src + dst + body + payload


def eth(rng, payload, et, tags=()):
    """Ethernet II with the given VLAN tag types in front of ethertype et"""
    ets = list(tags) + [et]
    out = rbytes(rng, 12) + be16(ets[0])
    for k in range(len(tags)):
        out += be16(rng.getrandbits(16)) + be16(ets[k + 1])
    return out + payload


def sll(rng, payload, et, tags=()):
    """Linux cooked capture (link type 113): 16 bytes, the protocol in the last two"""
    ets = list(tags) + [et]
    out = rbytes(rng, 14) + be16(ets[0])
    for k in range(len(tags)):
        out += be16(rng.getrandbits(16)) + be16(ets[k + 1])
    return out + payload


def ip(rng, l4, kind, proto, **kw):
    if kind == 4:
        return v4hdr(rng, l4, proto, **kw)
    return v6hdr(rng, l4, proto, **kw)


def pick_l4(rng, l4gen, tag):
    proto = 17 if rng.random() < 0.6 else 6
    return proto, l4gen(rng, proto, tag)


def plain_ip(rng, l4gen, tag, kind=None):
    """an intact IPv4 or IPv6 packet, (kind, bytes)"""
    kind = kind or rng.choice((4, 6))
    proto, l4 = pick_l4(rng, l4gen, tag)
    return kind, ip(rng, l4, kind, proto)


ET = {4: 0x0800, 6: 0x86DD}


# ---------------------------------------------------------------- families: each returns (kind, ip bytes) or a frame
def fam_l2(rng, l4gen, tag, **kw):
    """returns a whole Ethernet frame"""
    kind, pkt = plain_ip(rng, l4gen, tag)
    r = rng.random()
    if r < 0.08:
        return eth(rng, pkt, rng.choice((0x0000, 0x002E, 0x05DC, 0x05FF)))  # a length field: below 0x600
    if r < 0.18:
        return eth(rng, pkt, rng.choice((0x0600, 0x0806, 0x8847, 0x88CC, 0x86DE)))
    ntags = rng.choice((0, 1, 2, 3, 7, 8, 9)) if rng.random() < 0.7 else rng.randrange(0, 10)
    return eth(rng, pkt, ET[kind], [rng.choice((0x8100, 0x88A8)) for _ in range(ntags)])


def fam_ipv4(rng, l4gen, tag, **kw):
    proto = rng.choice((17, 17, 6, 6, 4, 41, 47))
    inner = l4gen(rng, proto if proto in (6, 17) else 17, tag)
    if proto in (4, 41):
        inner = ip(rng, inner, 4 if proto == 4 else 6, 17)
    kw = {}
    r = rng.random()
    if r < 0.25:
        kw["ihl"] = rng.randrange(5, 16)
    elif r < 0.33:
        kw["ihl"] = rng.randrange(0, 5)
    elif r < 0.40:
        kw["ver"] = rng.choice((0, 5, 6, 15))
    r = rng.random()
    if r < 0.5:
        kw["total"] = rng.choice(("zero", "below_hl", "hl", "below", "beyond"))
    r = rng.random()
    if r < 0.3:
        kw["frag"] = rng.choice((0x0000, 0x2000, 0x0001, 0x1FFF, 0x4001, 0x6000, 0x8000))
    return 4, v4hdr(rng, inner, proto, **kw)


def rand_chain(rng, n, maxlb=3):
    return [(t, 0 if t == 44 else rng.randrange(0, maxlb + 1)) for t in (rng.choice((0, 43, 44, 51, 60)) for _ in range(n))]


def fam_ipv6(rng, l4gen, tag, maxlb=3, **kw):
    proto, l4 = pick_l4(rng, l4gen, tag)
    r = rng.random()
    n = rng.choice((0, 1, 2, 7, 8, 9, 12)) if rng.random() < 0.6 else rng.randrange(0, 13)
    no_frag = [(t, lb) for t, lb in rand_chain(rng, n, maxlb) if t != 44]
    kw = {}
    if r < 0.45:
        chain = no_frag
    elif r < 0.55:  # a fragment header in the middle, another header after it: both walks forget it
        k = rng.randrange(0, len(no_frag)) if no_frag else 0
        chain = no_frag[:k] + [(44, 0), (rng.choice((0, 43, 51, 60)), rng.randrange(0, maxlb + 1))] + no_frag[k:]
    elif r < 0.65:  # a fragment header last
        chain = no_frag + [(44, 0)]
    elif r < 0.75:
        chain = no_frag or [(60, 0)]
        kw["past"] = True
    else:
        chain = rand_chain(rng, n, maxlb)
    if rng.random() < 0.35:
        kw["paylen"] = rng.choice(("zero", "short", "long"))
    return 6, v6hdr(rng, l4, proto, chain[:12], **kw)


def fam_tunnel(rng, l4gen, tag, **kw):
    depth = rng.choice((0, 1, 3, 4, 5, 6)) if rng.random() < 0.6 else rng.randrange(0, 7)
    kinds = [rng.choice((4, 6)) for _ in range(depth + 1)]
    proto, pkt = pick_l4(rng, l4gen, tag)
    bad_inner = depth > 0 and rng.random() < 0.12
    for i in range(depth, -1, -1):
        pkt = ip(rng, pkt, kinds[i], proto)
        if bad_inner and i == depth:
            pkt = bytes([(rng.choice((0, 5, 7, 15)) << 4) | (pkt[0] & 15)]) + pkt[1:]
        proto = 4 if kinds[i] == 4 else 41
    return kinds[0], pkt


def fam_l4(rng, l4gen, tag, **kw):
    return plain_ip(rng, l4gen, tag)


def fam_mixed(rng, l4gen, tag, **kw):
    return rng.choice((fam_ipv4, fam_ipv6, fam_tunnel, fam_l4))(rng, l4gen, tag, **kw)


IP_FAMILIES = {"ipv4": fam_ipv4, "ipv6": fam_ipv6, "tunnel": fam_tunnel, "l4": fam_l4}


def frames_of(rng, family, n, l4gen=fuzz_l4, linktype=1, maxlen=None, maxlb=3):
    """n frames of one family under one link type (maxlen: longer frames are drawn again; maxlb: the
    largest length byte of an IPv6 extension header)"""
    out = []
    while len(out) < n:
        if family == "l2":
            f = fam_l2(rng, l4gen, family)
        else:
            fn = IP_FAMILIES.get(family, fam_mixed)
            kind, pkt = fn(rng, l4gen, family, maxlb=maxlb)
            if linktype == 1:
                f = eth(rng, pkt, ET[kind], [0x8100] if rng.random() < 0.1 else ())
            elif linktype == 113:
                r = rng.random()
                et = ET[kind] if r < 0.85 else rng.choice((0x0806, 0x0004, 0x88CC))
                f = sll(rng, pkt, et, [rng.choice((0x8100, 0x88A8))] if rng.random() < 0.2 else ())
            else:  # raw IP, sometimes with a version nibble that is neither 4 nor 6
                f = pkt if rng.random() < 0.9 else bytes([(rng.choice((0, 5, 7)) << 4) | (pkt[0] & 15)]) + pkt[1:]
        if maxlen is None or len(f) <= maxlen:
            out.append(f)
    return out


def record(frame, caplen=None, sec=1_700_000_000, usec=0):
    cap = len(frame) if caplen is None else caplen
    return struct.pack("<IIII", sec, usec, cap, len(frame)) + frame[:cap]


def pcap(records, linktype=1):
    return struct.pack("<IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, 65535, linktype) + b"".join(records)


# ---------------------------------------------------------------- the frames of the issue's table
def tcp25(syn=False):
    return struct.pack(">HHIIBBHHH", 40000, 179, 1, 0, 5 << 4, 0x02 if syn else 0x18, 8192, 0, 0) + b"\xff" * 5


def ext_chain_frame(n, l4=None, proto=6):
    """Eth + IPv6 + n destination-option headers of 8 bytes + an L4 layer (a 25-byte TCP one)"""
    rng = random.Random(1)
    return eth(rng, v6hdr(rng, tcp25() if l4 is None else l4, proto, [(60, 0)] * n, src="2001:db8::1", dst="2101:db8::1"), 0x86DD)


def nested_v4_frame(k, l4=None, proto=6):
    """Eth + k IPv4 headers (protocol 4 between them) + an L4 layer (a 25-byte TCP one)"""
    rng = random.Random(2)
    pkt = tcp25() if l4 is None else l4
    for _ in range(k):
        pkt, proto = v4hdr(rng, pkt, proto, src="10.1.2.3", dst="8.8.8.8"), 4
    return eth(rng, pkt, 0x0800)
