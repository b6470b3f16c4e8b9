"""Hand-built TCP segments and BGP streams as classic-pcap records (test infrastructure; scapy and
dpkt are not installed): TCP headers over the link and IP builders of tests/dhcp_cases.py, BGP
messages, two-sided sessions, and the random stream corpus of the reassembly tests."""
import struct

import numpy as np

from tests.dhcp_cases import T0, eth, filler, ipv4, ipv6, record  # noqa: F401

FIN, SYN, RST, PSH, ACK = 1, 2, 4, 8, 16
A4, B4 = "10.0.0.1", "10.0.0.2"
A6 = bytes.fromhex("20010db8000000000000000000000001")
B6 = bytes.fromhex("20010db8000000000000000000000002")
MARKER = struct.pack("<IIII", 0xFFFFFFFF, 0, 0, 0)  # ends a stream in a corpus file (tests/native_bgp/bgp_asan_main.cpp)


def tcp(payload: bytes, sp: int, dp: int, seq: int = 1, flags: int = PSH | ACK, doff: int = 5, ack: int = 0) -> bytes:
    h = struct.pack(">HHIIBBHHH", sp, dp, seq & 0xFFFFFFFF, ack, doff << 4, flags, 8192, 0, 0)
    return h + bytes(max(0, doff * 4 - 20)) + payload


def bgp_msg(mtype: int, body: bytes = b"") -> bytes:
    """marker(16) length(2) type(1) body"""
    return b"\xff" * 16 + struct.pack(">HB", 19 + len(body), mtype) + body


def seg4(payload: bytes, sp: int, dp: int, seq: int, sec: int = T0, frac: int = 0, flags: int = PSH | ACK, src=A4, dst=B4,
         **kw) -> bytes:
    """one Ethernet / IPv4 / TCP record"""
    return record(eth(ipv4(tcp(payload, sp, dp, seq, flags), 6, src, dst, **kw)), sec, frac)


def seg6(payload: bytes, sp: int, dp: int, seq: int, sec: int = T0, frac: int = 0, flags: int = PSH | ACK, src=A6, dst=B6,
         **kw) -> bytes:
    return record(eth(ipv6(tcp(payload, sp, dp, seq, flags), 6, src, dst, **kw), 0x86DD), sec, frac)


def foreign(sec: int = T0, frac: int = 0, sp: int = 443, dp: int = 40000) -> bytes:
    """a TCP record of another port pair (an ACK without data: reassembly ignores it, the time-outs do not)"""
    return seg4(b"", sp, dp, 7, sec, frac, ACK, "10.1.0.1", "10.1.0.2")


class Peer:
    """one side of a session: sends messages in order from its own sequence number"""

    def __init__(self, sp, dp, seq, v6=False, src=None, dst=None):
        self.sp, self.dp, self.seq, self.v6 = sp, dp, seq & 0xFFFFFFFF, v6
        self.src = src or (A6 if v6 else A4)
        self.dst = dst or (B6 if v6 else B4)

    def send(self, payload: bytes, sec=T0, frac=0, flags=PSH | ACK, seq=None, advance=True) -> bytes:
        s = self.seq if seq is None else seq & 0xFFFFFFFF
        f = seg6 if self.v6 else seg4
        r = f(payload, self.sp, self.dp, s, sec, frac, flags, self.src, self.dst)
        if advance and seq is None:
            self.seq = (self.seq + len(payload) + (1 if flags & SYN else 0)) & 0xFFFFFFFF
        return r

    def skip(self, n: int):
        self.seq = (self.seq + n) & 0xFFFFFFFF


def session(port=40001, seq_a=1000, seq_b=5000, v6=False):
    """(client, server) of one connection to port 179"""
    if v6:
        return Peer(port, 179, seq_a, True, A6, B6), Peer(179, port, seq_b, True, B6, A6)
    return Peer(port, 179, seq_a, False, A4, B4), Peer(179, port, seq_b, False, B4, A4)


def opened(port=40001, sec=T0, seq_a=1000, seq_b=5000, v6=False):
    """(client, server, their two SYN records at sec): a connection whose first packet carries no
    data, so it is put into the LRU list with that packet's stamp"""
    a, b = session(port, seq_a, seq_b, v6)
    return a, b, a.send(b"", sec, 0, SYN) + b.send(b"", sec, 1, SYN | ACK)


def keepalive_stream(n: int, sec0: int = T0, step_us: int = 1000, port: int = 40001) -> bytes:
    """n records of one session: a SYN each way, then messages alternating between the sides with
    types cycling 1..5"""
    a, b = session(port)
    out, t = [], 0
    for i in range(n):
        s, us = sec0 + t // 1000000, t % 1000000
        p = a if i % 2 == 0 else b
        if i < 2:
            out.append(p.send(b"", s, us, SYN | (ACK if i else 0)))
        else:
            out.append(p.send(bgp_msg(1 + i % 5, bytes(i % 7)), s, us))
        t += step_us
    return b"".join(out)


def shapes():
    """frame shapes of the general parse path, each one BGP segment unless noted: {name: (linktype, records, segments)}"""
    m = bgp_msg(2, b"shape")
    t = tcp(m, 40001, 179, 10)
    c = {}
    c["vlan"] = (1, record(eth(ipv4(t, 6, A4, B4), vlan=7)), 1)
    c["qinq"] = (1, record(A6[:6] + B6[:6] + bytes.fromhex("88a80005") + bytes.fromhex("81000006") + b"\x08\x00"
                              + ipv4(t, 6, A4, B4)), 1)
    c["v6"] = (1, seg6(m, 179, 40001, 10), 1)
    c["v6_hop_by_hop"] = (1, record(eth(ipv6(t, 6, A6, B6, hop_by_hop=True), 0x86DD)), 1)
    c["ihl6_ihl10_ihl12"] = (1, b"".join(record(eth(ipv4(t, 6, A4, B4, ihl=k)), T0, k) for k in (6, 10, 12)), 3)
    frame = eth(ipv4(t, 6, A4, B4))
    # cut inside the payload (IP total beyond the capture), at the TCP header's end, inside the TCP header
    c["caplen_cut"] = (1, record(frame, caplen=len(frame) - 9) + record(frame, T0, 1, caplen=54) + record(frame, T0, 2, caplen=50), 1)
    c["raw_ip"] = (101, record(ipv4(t, 6, A4, B4)) + record(ipv6(t, 6, A6, B6), T0, 1), 2)
    c["tcp_options"] = (1, record(eth(ipv4(tcp(m, 40001, 179, 10, doff=8), 6, A4, B4))), 1)
    # data offset 4 (no TcpLayer), data offset past the layer, a pure ACK, a fragment, another port
    c["not_segments"] = (1, record(eth(ipv4(tcp(m, 40001, 179, 10, doff=4), 6, A4, B4)))
                         + record(eth(ipv4(tcp(b"", 40001, 179, 10, doff=5)[:12] + b"\xf0" + tcp(b"", 1, 1)[13:], 6, A4, B4)))
                         + seg4(b"", 40001, 179, 10, flags=ACK) + record(eth(ipv4(t, 6, A4, B4, frag=0x2000)))
                         + seg4(m, 40001, 180, 10) + filler(), 0)
    c["flags_only"] = (1, seg4(b"", 40001, 179, 10, flags=SYN) + seg4(b"", 179, 40001, 10, T0, 1, FIN | ACK, B4, A4)
                       + seg4(b"", 40001, 179, 11, T0, 2, RST), 3)
    c["v4_in_v6_tunnel"] = (1, record(eth(ipv6(ipv4(t, 6, A4, B4), 4, A6, B6), 0x86DD)), 1)
    return c


def random_stream(rng, kind: int = 0):
    """One random capture as a list of records: up to three port-179 connections whose two sides'
    in-order segment lists are perturbed (drops of 1, 10, 100 and random bytes, duplicates,
    reorderings, backwards-extended retransmissions), interleaved, stamped with small steps and
    now and then 29 / 30 / 31 s or 299 / 300 s jumps, with foreign TCP and UDP records between.
    kind 1: more than 50 held fragments; kind 2: a side change while fragments are held."""
    tracks = []
    for c in range(int(rng.integers(1, 4))):
        v6 = bool(rng.integers(0, 4) == 0)
        wrap = rng.integers(0, 3) == 0
        a, b = session(40000 + c, 0xFFFFFF00 + int(rng.integers(0, 256)) if wrap else int(rng.integers(0, 1 << 32)),
                       int(rng.integers(0, 1 << 32)), v6)
        for p in (a, b):
            segs = []
            if rng.integers(0, 5):
                segs.append(("syn", p.seq, bgp_msg(1) if rng.integers(0, 5) == 0 else b"", SYN))
                p.skip(len(segs[-1][2]) + 1)
            nmsg = int(rng.integers(0, 9)) if kind != 1 else int(rng.integers(53, 62))
            for i in range(nmsg):
                r = int(rng.integers(0, 10))
                mtype = int(rng.choice([0, 1, 2, 3, 4, 5, 6]))
                if r == 0:
                    pay = bgp_msg(mtype)[:18]
                elif r == 1:
                    pay = bgp_msg(mtype)
                elif r == 2:
                    pay = bgp_msg(mtype, b"x") + bgp_msg(4) + bgp_msg(2, b"yy")  # three messages, one chunk
                elif r == 3:
                    pay = bytes([mtype]) * int(rng.integers(1, 40))  # byte 18 is the type, or absent
                else:
                    pay = bgp_msg(mtype, rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8).tobytes())
                segs.append(("data", p.seq, pay, PSH | ACK))
                p.skip(len(pay))
                if kind == 1 and i == 0:
                    segs[-1] = ("drop",) + segs[-1][1:]
                elif rng.integers(0, 7) == 0:
                    # a hole in the sequence space: its text is 17, 18 or 19 and more characters
                    p.skip(int(rng.choice([1, 10, 100, int(rng.integers(1, 3000))])))
            out = []
            for j, (what, seq, pay, fl) in enumerate(segs):
                r = int(rng.integers(0, 20)) if what == "data" and kind != 1 else 99
                if what == "drop" or r == 0:
                    continue
                out.append((seq, pay, fl))
                if r == 1:
                    out.append((seq, pay, fl))  # a duplicate
                elif r == 2 and j:
                    k = int(rng.integers(1, 12))  # a retransmission that starts k bytes early
                    out.append(((seq - k) & 0xFFFFFFFF, bytes([1 + k % 5]) * k + pay, fl))
                elif r == 3 and len(pay) > 4:
                    out.append(((seq + 2) & 0xFFFFFFFF, pay[2:] + bgp_msg(3), fl))  # overlaps and reaches past
            for j in range(len(out) - 1):
                if rng.integers(0, 6) == 0:
                    k = min(len(out) - 1, j + int(rng.integers(1, 4)))
                    out[j], out[k] = out[k], out[j]
            end = int(rng.integers(0, 6))
            if end == 1:
                out.append((p.seq, b"", FIN | ACK))
            elif end == 2:
                out.append((p.seq, b"", RST))
            elif end == 3:
                out.append((p.seq, bgp_msg(3), FIN | PSH | ACK))
            elif end == 4:
                out.insert(int(rng.integers(0, len(out) + 1)), (p.seq, b"", FIN | ACK))  # data after a FIN is ignored
            tracks.append((p, out))
    if kind == 2:
        # side A leaves a fragment held, then side B speaks: A's fragment is flushed behind a text
        a, b = session(40009, 100, 900)
        tracks.append((a, [(100, bgp_msg(1), PSH | ACK), (100 + 19 + int(rng.choice([1, 10, 100])), bgp_msg(2, b"held"), PSH | ACK)]))
        tracks.append((b, [(900, bgp_msg(4), PSH | ACK)]))
    recs, sec, us = [], T0 + int(rng.integers(0, 100)), int(rng.integers(0, 1000000))
    order = []
    for ti, (_p, out) in enumerate(tracks):
        order += [ti] * len(out)
    if kind == 2:
        order = order[:-3] + sorted(order[-3:])
    else:
        rng.shuffle(order)
    nxt = [0] * len(tracks)
    for ti in order:
        r = int(rng.integers(0, 40))
        if r == 0:
            sec += int(rng.choice([29, 30, 31]))
        elif r == 1:
            sec += int(rng.choice([299, 300, 331]))
        else:
            us += int(rng.integers(0, 3000))
            sec, us = sec + us // 1000000, us % 1000000
        if r < 6:
            recs.append(foreign(sec, us) if r % 2 == 0 else filler(sec, us))
            us = min(999999, us + 1)
        p, out = tracks[ti]
        seq, pay, fl = out[nxt[ti]]
        nxt[ti] += 1
        recs.append(p.send(pay, sec, us, fl, seq=seq))
    if rng.integers(0, 3) == 0:
        recs.append(foreign(sec + int(rng.choice([1, 29, 30, 31])), us))
    return recs


def corpus(n: int, seed: int):
    """n random streams (lists of records); every 16th has more than 50 held fragments, every 16th a
    side change with held fragments"""
    rng = np.random.default_rng(seed)
    return [random_stream(rng, 1 if i % 16 == 5 else (2 if i % 16 == 11 else 0)) for i in range(n)]
