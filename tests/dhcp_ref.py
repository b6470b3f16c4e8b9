"""Python model of the DHCP handler (test infrastructure): an independent restatement of the
decoder rules of pktvisor_amd/csrc/pv_dhcp.h and of DhcpMetricsManager / DhcpMetricsBucket
(src/handlers/dhcp/DhcpStreamHandler.cpp) over classic-pcap records: record walk, UDP location
(the Net pass's meaning of "a UDP packet"), decode, manager, JSON. Precedent: tests/mmdb_ref.py."""
import math
import socket
import struct


class Jsf32:
    """jsf32 with the reference's default seed (3rd/rng/jsf.h); its first draws are pinned by
    tests/golden/jsf32_seed1.json, which tests/gen_jsf32.py writes from the reference's generator"""

    def __init__(self):
        self.a, self.b, self.c, self.d = 0xf1ea5eed, 1, 1, 1
        for _ in range(20):
            self.next()

    @staticmethod
    def _rot(x, k):
        return ((x << k) | (x >> (32 - k))) & 0xFFFFFFFF

    def next(self):
        e = (self.a - self._rot(self.b, 27)) & 0xFFFFFFFF
        self.a = self.b ^ self._rot(self.c, 17)
        self.b = (self.c + self.d) & 0xFFFFFFFF
        self.c = (self.d + e) & 0xFFFFFFFF
        self.d = (e + self.a) & 0xFFFFFFFF
        return self.d


def records(recs: bytes):
    """(offset, sec, frac, caplen) of every whole record"""
    pos, out = 0, []
    while pos + 16 <= len(recs):
        sec, frac, cap, _ = struct.unpack_from("<IIII", recs, pos)
        if pos + 16 + cap > len(recs):
            break
        out.append((pos, sec, frac, cap))
        pos += 16 + cap
    return out


def be16(b, o):
    return (b[o] << 8) | b[o + 1] if o + 1 < len(b) else ((b[o] << 8) if o < len(b) else 0)


def locate_udp(frame: bytes, linktype: int):
    """The UDP layer as PcapPlusPlus / the Net pass see it: (l4off, l4len, first IPv4 offset or
    None, first IPv6 offset or None), or None when the packet has no UDP layer. Offsets are into
    frame; l4len is trimmed by the IP lengths."""
    cur, ln, kind = 0, len(frame), 0
    if linktype == 1:
        if ln < 14:
            return None
        et = be16(frame, 12)
        if not (et >= 0x600 and ln > 14):
            return None
        cur, ln = 14, ln - 14
        d = 0
        while d < 8 and et in (0x8100, 0x88A8):
            if ln <= 4:
                return None
            et = be16(frame, cur + 2)
            cur, ln, d = cur + 4, ln - 4, d + 1
        kind = 4 if et == 0x0800 else (6 if et == 0x86DD else 0)
    elif linktype == 113:
        if ln <= 16:
            return None
        et = be16(frame, 14)
        cur, ln = 16, ln - 16
        d = 0
        while d < 8 and et in (0x8100, 0x88A8):
            if ln <= 4:
                return None
            et = be16(frame, cur + 2)
            cur, ln, d = cur + 4, ln - 4, d + 1
        kind = 4 if et == 0x0800 else (6 if et == 0x86DD else 0)
    elif linktype in (101, 12, 14, 228, 229):
        if ln >= 1:
            v = frame[0] >> 4
            kind = v if v in (4, 6) else 0
    v4 = v6 = None
    for _ in range(5):  # five IP headers, as the oracle walks
        if not kind:
            return None
        if kind == 4:
            if ln < 20:
                return None
            b0 = frame[cur]
            if (b0 >> 4) != 4 or (b0 & 15) < 5:
                return None
            if v4 is None:
                v4 = cur
            total = be16(frame, cur + 2)
            if total < ln and total != 0:
                ln = total
            hl = (b0 & 15) * 4
            if ln <= hl:
                return None
            if be16(frame, cur + 6) & 0x3fff:
                return None
            proto = frame[cur + 9]
        else:
            if ln < 40:
                return None
            if v6 is None:
                v6 = cur
            nxt, off, frag = frame[cur + 6], 40, False
            while ln >= 2 and off <= ln - 2:  # bounded by the length alone
                if nxt == 44:
                    elen = 8
                elif nxt in (0, 60, 43):
                    elen = (frame[cur + off + 1] + 1) * 8
                elif nxt == 51:
                    elen = (frame[cur + off + 1] + 2) * 4
                else:
                    break
                frag = nxt == 44
                nxt = frame[cur + off]
                off += elen
            total = be16(frame, cur + 4) + off
            if total < ln:
                ln = total
            hl = off
            if ln <= hl or frag:
                return None
            proto = nxt
        pl, pll = cur + hl, ln - hl
        if proto == 17:
            return (pl, pll, v4, v6) if pll >= 8 else None
        if proto == 6:
            return None
        if proto in (4, 41) and pll >= 1:
            v = frame[pl] >> 4
            kind = v if v in (4, 6) else 0
            cur, ln = pl, pll
            continue
        return None
    return None


def decode_record(rec: bytes, index: int, linktype: int = 1, ts_nano: int = 0):
    """One pcap record (16-byte header + captured bytes) -> the event dict, or None"""
    sec, frac, cap, _ = struct.unpack_from("<IIII", rec, 0)
    frame = rec[16:16 + cap]
    u = locate_udp(frame, linktype)
    if u is None:
        return None
    l4off, l4len, _v4, v6 = u
    sp, dp = be16(frame, l4off), be16(frame, l4off + 2)
    if sp in (67, 68) or dp in (67, 68):
        fam = 4
    elif sp in (546, 547) or dp in (546, 547):
        fam = 6
    else:
        return None
    pay = frame[l4off + 8:l4off + l4len]  # (a slice clips to the captured bytes)
    ev = {"rec": index, "sec": sec, "nsec": frac if ts_nano else frac * 1000, "family": fam, "mtype": 0, "xid": 0,
          "yiaddr": b"\0\0\0\0", "server": None, "cmac": bytes(6), "emac": None, "v6src": None, "hostname": None}
    if linktype == 1:
        ev["emac"] = bytes(frame[6:12])
    if v6 is not None:
        ev["v6src"] = bytes(frame[v6 + 8:v6 + 24])
    if fam == 4:
        if len(pay) < 240:
            return ev
        ev["xid"] = struct.unpack_from("<I", pay, 4)[0]
        ev["yiaddr"] = bytes(pay[16:20])
        if pay[1] == 1 and pay[2] == 6:
            ev["cmac"] = bytes(pay[28:34])
        seen, pos = {}, 240
        while pos < len(pay):
            t = pay[pos]
            if t in (0, 255):
                pos += 1
                continue
            if pos + 2 > len(pay):
                break
            ln = pay[pos + 1]
            if pos + 2 + ln > len(pay):
                break
            seen.setdefault(t, bytes(pay[pos + 2:pos + 2 + ln]))
            pos += 2 + ln
        if 53 in seen and seen[53]:
            ev["mtype"] = seen[53][0]
        if 12 in seen:
            ev["hostname"] = seen[12]
        if 54 in seen:
            ev["server"] = seen[54][:4] if len(seen[54]) >= 4 else b"\0\0\0\0"
    else:
        if not pay:
            return ev
        ev["mtype"] = pay[0]
        pos = 4
        while pos + 4 <= len(pay):
            t, ln = be16(pay, pos), be16(pay, pos + 2)
            if t == 2:
                ev["server"] = b""
                break
            pos += 4 + ln
    return ev


def decode(recs: bytes, linktype: int = 1, ts_nano: int = 0):
    out = []
    for i, (pos, _s, _f, cap) in enumerate(records(recs)):
        ev = decode_record(recs[pos:pos + 16 + cap], i, linktype, ts_nano)
        if ev is not None:
            out.append(ev)
    return out


def mac_text(m: bytes) -> str:
    return ":".join(f"{x:02x}" for x in m)


def ip4_text(a: bytes) -> str:
    return ".".join(str(x) for x in a)


COUNTERS = ("events", "deep_samples", "discover", "offer", "request", "ack", "solicit", "advertise", "request_v6", "reply",
            "total", "filtered")


class Bucket:
    def __init__(self, sec=0, nsec=0):
        self.start, self.end = (sec, nsec), (0, 0)
        self.read_only, self.length = False, 0
        self.c = {k: 0 for k in COUNTERS}
        self.clients, self.servers = {}, {}


class Manager:
    """DhcpMetricsManager with its own window, jsf32 draws and request/ack transactions"""

    def __init__(self, num_periods=5, deep_sample_rate=100, xact_ttl_ms=5000, topn_count=10, topn_percentile_threshold=0):
        self.num_periods = num_periods
        self.rate = deep_sample_rate or 100
        ttl = xact_ttl_ms or 5000
        self.ttl_s, self.ttl_ms = (ttl // 1000, ttl % 1000) if ttl > 1000 else (0, ttl)
        self.topn, self.pct = topn_count, topn_percentile_threshold
        self.reset()

    def reset(self):
        self.buckets = [Bucket()]
        self.xact = {}
        self.rng = Jsf32()
        self.deep = True
        self.started = False
        self.next_shift = 0

    def set_start(self, sec, nsec):
        if self.started:
            return
        self.buckets[0].start = (sec, nsec)
        self.next_shift = sec + 60
        self.started = True

    def set_end(self, sec, nsec):
        b = self.buckets[0]
        b.end, b.length, b.read_only = (sec, nsec), sec - b.start[0], True

    def _shift(self, sec, nsec):
        p = self.buckets[0]
        p.end, p.length, p.read_only = (sec, nsec), sec - p.start[0], True
        self.buckets.insert(0, Bucket(sec, nsec))
        del self.buckets[self.num_periods:]
        self.next_shift = sec + 60
        self.xact = {k: v for k, v in self.xact.items() if not sec >= self.ttl_s + v[0]}

    def check_period_shift(self, sec, nsec=0):
        if self.started and self.num_periods > 1 and sec >= self.next_shift:
            self._shift(sec, nsec)

    def feed(self, recs: bytes, linktype: int = 1, ts_nano: int = 0):
        """one batch: the input's start stamp is its first record's"""
        rs = records(recs)
        if not rs:
            return
        self.set_start(rs[0][1], rs[0][2] if ts_nano else rs[0][2] * 1000)
        for ev in decode(recs, linktype, ts_nano):
            self.event(ev)

    def event(self, ev):
        sec, nsec = ev["sec"], ev["nsec"]
        if self.rate != 100:
            self.deep = self.rng.next() % 100 < self.rate
        if self.num_periods > 1 and sec >= self.next_shift:
            self._shift(sec, nsec)
        b, deep = self.buckets[0], self.deep
        b.c["events"] += 1
        if deep:
            b.c["deep_samples"] += 1
        t = ev["mtype"]
        if ev["family"] == 4:
            b.c["total"] += 1
            name = {1: "discover", 2: "offer", 3: "request", 5: "ack"}.get(t)
            if name:
                b.c[name] += 1
            if deep and t == 2 and ev["server"] is not None and ev["emac"] is not None:
                k = mac_text(ev["emac"]) + "/" + ip4_text(ev["server"])
                b.servers[k] = b.servers.get(k, 0) + 1
            if t == 3:
                host = b"Unknown" if ev["hostname"] is None else ev["hostname"]
                self.xact[ev["xid"]] = (sec, nsec, host, mac_text(ev["cmac"]))
            elif t == 5 and ev["xid"] in self.xact:
                s0, n0, host, mac = self.xact.pop(ev["xid"])
                ds = sec - s0 if sec > s0 else s0 - sec
                dn = nsec - n0
                if dn < 0:
                    ds, dn = ds - 1, dn + 1000000000
                timed_out = ds > self.ttl_s or (ds == self.ttl_s and dn / 1.0e6 >= self.ttl_ms)
                if not timed_out and deep and ev["yiaddr"] != b"\0\0\0\0":
                    k = mac + "/" + host.decode("latin-1") + "/" + ip4_text(ev["yiaddr"])
                    b.clients[k] = b.clients.get(k, 0) + 1
        else:
            name = {1: "solicit", 2: "advertise", 3: "request_v6", 7: "reply"}.get(t)
            if name:
                b.c[name] += 1
            if (deep and t in (2, 7) and ev["server"] is not None and ev["emac"] is not None and ev["v6src"] is not None
                    and ev["v6src"] != bytes(16)):
                k = mac_text(ev["emac"]) + "/" + socket.inet_ntop(socket.AF_INET6, ev["v6src"])
                b.servers[k] = b.servers.get(k, 0) + 1

    def _top(self, m):
        v = sorted(m.items(), key=lambda kv: (-kv[1], kv[0].encode("latin-1")))[:self.topn]
        if not v:
            return []
        est = sorted(c for _, c in v)
        w = math.ceil(self.pct / 100.0 * len(v))
        thr = est[0 if w == 0 else min(w - 1, len(v) - 1)]
        out = []
        for name, c in v:
            if c < thr:
                break
            out.append({"name": name, "estimate": c})
        return out

    def window(self, period=0, merged=False) -> dict:
        """the "dhcp" object of window_json (names: bytes as latin-1 characters, as the JSON's \\u00XX read)"""
        if not merged:
            bs = [self.buckets[period]]
        else:
            bs = self.buckets[:period]
        c = {k: sum(b.c[k] for b in bs) for k in COUNTERS}
        clients, servers = {}, {}
        for b in bs:
            for k, v in b.clients.items():
                clients[k] = clients.get(k, 0) + v
            for k, v in b.servers.items():
                servers[k] = servers.get(k, 0) + v
        return {"period": {"start_ts": min(b.start[0] for b in bs), "length": sum(b.length for b in bs if b.read_only)},
                "wire_packets": c, "top_clients": self._top(clients), "top_servers": self._top(servers)}


def prometheus(win: dict, labels: str = "{}") -> str:
    """DhcpMetricsBucket::to_prometheus of a window() result (no added labels by default)"""
    help_ = [("events", "Total DHCP wire packets events"),
             ("deep_samples", "Total DHCP wire packets that were sampled for deep inspection"),
             ("discover", "Total DHCP packets with message type DISCOVER"), ("offer", "Total DHCP packets with message type OFFER"),
             ("request", "Total DHCP packets with message type REQUEST"), ("ack", "Total DHCP packets with message type ACK"),
             ("solicit", "Total DHCPv6 packets with message type SOLICIT"),
             ("advertise", "Total DHCPv6 packets with message type ADVERTISE"),
             ("request_v6", "Total DHCPv6 packets with message type REQUEST"),
             ("reply", "Total DHCPv6 packets with message type REPLY"),
             ("total", "Total DHCP/DHCPv6 wire packets matching the configured filter(s)"),
             ("filtered", "Total DHCP/DHCPv6 wire packets seen that did not match the configured filter(s) (if any)")]
    out = []
    for k, h in help_:
        n = "dhcp_wire_packets_" + k
        out.append(f"# HELP {n} {h}\n# TYPE {n} gauge\n{n}{labels} {win['wire_packets'][k]}\n")
    for key, item, h in (("top_clients", "client", "Top DHCP clients"), ("top_servers", "server", "Top DHCP servers")):
        if not win[key]:
            continue
        n = "dhcp_" + key
        out.append(f"# HELP {n} {h}\n# TYPE {n} gauge\n")
        for e in win[key]:
            out.append(f'{n}{{{item}="{e["name"]}"}} {e["estimate"]}\n')
    return "".join(out)
