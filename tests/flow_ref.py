"""Python model of the flow handler (test infrastructure): an independent restatement of the
datagram check (process_netflow_packet, src/inputs/flow/NetflowData.h:59-213,678-699) and of
FlowStreamHandler::process_netflow_cb / FlowMetricsBucket (src/handlers/flow/FlowStreamHandler.cpp:
393-460,1056-1451) over classic-pcap records: record walk, UDP location (the Net pass's meaning of
"a UDP packet", tests/dhcp_ref.py), decode, manager, JSON. Cardinalities are exact distinct counts:
every case keeps at most 64 distinct values per sketch, where the sketch's rounded estimate is the
count (tests/test_flow_host.py checks that against the reference's sketch)."""
import math
import socket
import struct

from tests.dhcp_ref import Jsf32, locate_udp, records

HDR = {1: 16, 5: 24, 7: 24}
REC = {1: 48, 5: 48, 7: 52}
MAXFLOWS = {1: 24, 5: 30, 7: 30}
DEFAULT_GROUPS = ("counters", "cardinality", "top_ips", "top_ports", "top_ips_ports", "by_bytes", "by_packets")
ALL_GROUPS = DEFAULT_GROUPS + ("conversations", "top_tos", "top_geo", "top_interfaces")
DSCP = {0: "CS0", 8: "CS1", 16: "CS2", 24: "CS3", 32: "CS4", 40: "CS5", 48: "CS6", 56: "CS7", 10: "AF11", 12: "AF12", 14: "AF13",
        18: "AF21", 20: "AF22", 22: "AF23", 26: "AF31", 28: "AF32", 30: "AF33", 34: "AF41", 36: "AF42", 38: "AF43", 46: "EF",
        43: "VOICE-ADMIT"}
ECN = {0: "Not-ECT", 1: "ECT(1)", 2: "ECT(0)", 3: "CE"}
TYPES = (("in", "bytes"), ("out", "bytes"), ("in", "packets"), ("out", "packets"))  # FlowDirectionType
KINDS = ("udp_", "tcp_", "other_l4_", "ipv4_", "ipv6_", "")
TOPS = ("src_ips", "dst_ips", "src_ports", "dst_ports", "src_ip_ports", "dst_ip_ports", "dscp", "ecn")
TOP_GROUP = ("top_ips", "top_ips", "top_ports", "top_ports", "top_ips_ports", "top_ips_ports", "top_tos", "top_tos")
CARDS = ("conversations", "src_ips_in", "dst_ips_out", "src_ports_in", "dst_ports_out")


def groups_of(cfg: dict):
    """process_groups over the flow handler's defaults"""
    g = set(DEFAULT_GROUPS)
    for name in cfg.get("disable", []):
        if name == "all":
            g = set()
            break
        g.discard(name)
    for name in cfg.get("enable", []):
        if name == "all":
            g = set(ALL_GROUPS)
            break
        g.add(name)
    return g


def check(payload: bytes):
    """(version, count) of an accepted payload, else (version or 0, 0)"""
    if len(payload) < 4:
        return 0, 0
    version, count = struct.unpack_from(">HH", payload, 0)
    if version not in HDR:
        return version, 0
    if count == 0 or count > MAXFLOWS[version] or len(payload) != HDR[version] + count * REC[version]:
        return version, 0
    return version, count


def decode(recs: bytes, linktype: int = 1, ts_nano: int = 0, ports=()):
    """(datagrams, stats): every accepted datagram in record order as a dict, and the input's counts"""
    out, stats = [], {"datagrams": 0, "invalid": 0, "invalid_v9_v10": 0}
    for index, (pos, sec, frac, cap) in enumerate(records(recs)):
        frame = recs[pos + 16:pos + 16 + cap]
        loc = locate_udp(frame, linktype)
        if loc is None:
            continue
        l4off, l4len, v4, v6 = loc
        if l4len < 8:
            continue
        dport = (frame[l4off + 2] << 8) | frame[l4off + 3]
        if ports and dport not in ports:
            continue
        payload = frame[l4off + 8:l4off + l4len]  # (the slice clips to the captured bytes)
        version, count = check(payload)
        if not count:
            stats["invalid"] += 1
            if version in (9, 10):
                stats["invalid_v9_v10"] += 1
            continue
        stats["datagrams"] += 1
        if v4 is not None:
            device = socket.inet_ntop(socket.AF_INET, frame[v4 + 12:v4 + 16])
        else:
            device = socket.inet_ntop(socket.AF_INET6, frame[v6 + 8:v6 + 24])
        tsec, tnsec = struct.unpack_from(">II", payload, 8)
        flows = []
        for j in range(count):
            at = HDR[version] + j * REC[version]
            src, dst = payload[at:at + 4], payload[at + 4:at + 8]
            if_in, if_out, pkts, octets = struct.unpack_from(">HHII", payload, at + 12)
            sport, dport_ = struct.unpack_from(">HH", payload, at + 32)
            flows.append(dict(src=src, dst=dst, if_in=if_in, if_out=if_out, packets=pkts, octets=octets, sport=sport, dport=dport_,
                              proto=payload[at + 38], tos=payload[at + 39]))
        stamp = (tsec, tnsec) if (tsec or tnsec) else (sec, frac if ts_nano else frac * 1000)
        out.append(dict(rec=index, device=device, stamp=stamp, version=version, flows=flows))
    return out, stats


class PortNames:
    """IpPort's two lists and get_service (src/IpPort.cpp:11-32) over rows (last, first, protocol, name)"""

    def __init__(self, rows=()):
        self.lists = {6: {}, 17: {}}
        for last, first, proto, name in rows:
            self.lists[proto].setdefault(last, (name, first))
        self.keys = {p: sorted(m) for p, m in self.lists.items()}

    def service(self, port: int, udp: bool) -> str:
        proto = 17 if udp else 6
        for k in self.keys[proto]:  # lower_bound
            if k >= port:
                name, first = self.lists[proto][k]
                return name if (k == port or port >= first) else str(port)
        return str(port)


class Interface:
    def __init__(self):
        self.counters = [[0] * 6 for _ in TYPES]
        self.card = [set() for _ in CARDS]
        self.top = [[{} for _ in TOPS] for _ in TYPES]
        self.conv = [{}, {}]


class Device:
    def __init__(self):
        self.flows = 0
        self.top_if = [{} for _ in TYPES]
        self.ifs = {}


class Bucket:
    def __init__(self, sec=0, nsec=0):
        self.start, self.end = (sec, nsec), (0, 0)
        self.read_only, self.length = False, 0
        self.events = self.deep = 0
        self.devices = {}


def _add(m: dict, key, w: int):
    if w:  # a weight of 0 never enters a frequent-items sketch
        m[key] = m.get(key, 0) + w


def ip_text(a: bytes) -> str:
    return ".".join(str(x) for x in a)


class Manager:
    def __init__(self, num_periods=5, deep_sample_rate=100, cfg=None, port_rows=(), topn_count=10, topn_percentile_threshold=0,
                 ports=None):
        self.num_periods = num_periods
        self.rate = deep_sample_rate or 100
        self.g = groups_of(cfg or {})
        self.ports = tuple((cfg or {}).get("ports", ())) if ports is None else tuple(ports)
        self.names = PortNames(port_rows)
        self.topn, self.pct = topn_count, topn_percentile_threshold
        self.stats = {"datagrams": 0, "invalid": 0, "invalid_v9_v10": 0}
        self.reset()

    def reset(self):
        self.buckets = [Bucket()]
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
        if not self.started:
            return
        b = self.buckets[0]
        b.end, b.length, b.read_only = (sec, nsec), sec - b.start[0], True

    def _shift(self, sec, nsec):
        p = self.buckets[0]
        p.end, p.length, p.read_only = (sec, nsec), sec - p.start[0], True
        self.buckets.insert(0, Bucket(sec, nsec))
        del self.buckets[self.num_periods:]
        self.next_shift = sec + 60

    def check_period_shift(self, sec, nsec=0):
        if self.started and self.num_periods > 1 and sec >= self.next_shift:
            self._shift(sec, nsec)

    def feed(self, recs: bytes, linktype: int = 1, ts_nano: int = 0):
        """one batch: the input's start stamp is its first record's"""
        rs = records(recs)
        if not rs:
            return
        self.set_start(rs[0][1], rs[0][2] if ts_nano else rs[0][2] * 1000)
        dgrams, st = decode(recs, linktype, ts_nano, self.ports)
        for k, v in st.items():
            self.stats[k] += v
        for d in dgrams:
            self.datagram(d)

    def datagram(self, d):
        sec, nsec = d["stamp"]
        if self.rate != 100:
            self.deep = self.rng.next() % 100 < self.rate
        if self.num_periods > 1 and sec >= self.next_shift:
            self._shift(sec, nsec)
        b, g = self.buckets[0], self.g
        b.events += 1
        if self.deep:
            b.deep += 1
        dev = b.devices.setdefault(d["device"], Device())
        for f in d["flows"]:
            if "counters" in g:
                dev.flows += 1
            for out in (0, 1):
                idx = f["if_out"] if out else f["if_in"]
                ifc = dev.ifs.setdefault(idx, Interface())
                for pk in (0, 1):
                    if ("by_packets" if pk else "by_bytes") not in g:
                        continue
                    t = 2 * pk + out
                    self.interface(ifc, f, t)
                    if self.deep and "top_interfaces" in g:
                        _add(dev.top_if[t], str(idx), f["packets"] if pk else f["octets"])

    def interface(self, ifc, f, t):
        g = self.g
        agg = f["octets"] if t < 2 else f["packets"]
        if "counters" in g:
            c = ifc.counters[t]
            c[5] += agg
            c[3] += agg
            c[0 if f["proto"] == 17 else 1 if f["proto"] == 6 else 2] += agg
        if not self.deep:
            return
        udp = f["proto"] == 17
        sp, dp = str(f["sport"]), str(f["dport"])
        if "top_ports" in g:
            if f["sport"] > 0:
                sp = self.names.service(f["sport"], udp)
                _add(ifc.top[t][2], sp, agg)
            if f["dport"] > 0:
                dp = self.names.service(f["dport"], udp)
                _add(ifc.top[t][3], dp, agg)
        if "cardinality" in g:
            if f["sport"] > 0:
                ifc.card[3].add(f["sport"])
            if f["dport"] > 0:
                ifc.card[4].add(f["dport"])
        if "top_tos" in g:
            _add(ifc.top[t][6], DSCP.get(f["tos"] >> 2, str(f["tos"] >> 2)), agg)
            _add(ifc.top[t][7], ECN[f["tos"] & 3], agg)
        app = ["", ""]
        for side, key in ((0, "src"), (1, "dst")):
            a = f[key]
            if a == bytes(4):
                continue
            if "cardinality" in g:
                ifc.card[1 + side].add(a)
            ip = ip_text(a)
            port = f["dport"] if side else f["sport"]
            app[side] = ip + ":" + (dp if side else sp)
            if "top_ips" in g:
                _add(ifc.top[t][side], ip, agg)
            if port > 0 and "top_ips_ports" in g:
                _add(ifc.top[t][4 + side], app[side], agg)
        if "conversations" in g and f["sport"] > 0 and f["dport"] > 0 and app[0] and app[1]:
            conv = app[1] + "/" + app[0] if app[0] > app[1] else app[0] + "/" + app[1]
            if "cardinality" in g:
                ifc.card[0].add(conv)
            _add(ifc.conv[0 if t < 2 else 1], conv, agg)

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
        """the "flow" object of window_json"""
        bs = self.buckets[:period] if merged else [self.buckets[period]]
        g = self.g
        out = {"period": {"start_ts": min(b.start[0] for b in bs), "length": sum(b.length for b in bs if b.read_only)},
               "wire_packets": {"events": sum(b.events for b in bs), "deep_samples": sum(b.deep for b in bs)}}
        # the fold
        devices = {}
        for b in bs:
            for name, d in b.devices.items():
                o = devices.setdefault(name, Device())
                o.flows += d.flows
                for t in range(4):
                    for k, v in d.top_if[t].items():
                        _add(o.top_if[t], k, v)
                for idx, i in d.ifs.items():
                    oi = o.ifs.setdefault(idx, Interface())
                    for t in range(4):
                        for q in range(6):
                            oi.counters[t][q] += i.counters[t][q]
                        for q in range(len(TOPS)):
                            for k, v in i.top[t][q].items():
                                _add(oi.top[t][q], k, v)
                    for q in range(len(CARDS)):
                        oi.card[q] |= i.card[q]
                    for q in range(2):
                        for k, v in i.conv[q].items():
                            _add(oi.conv[q], k, v)
        devs = {}
        for name in sorted(devices):
            d, ds = devices[name], {}
            if "counters" in g:
                ds["records_flows"], ds["records_filtered"] = d.flows, 0
            if "top_interfaces" in g:
                for t, (dr, metric) in enumerate(TYPES):
                    if "by_" + metric in g:
                        ds[f"top_{dr}_interfaces_{metric}"] = self._top(d.top_if[t])
            ifs = {}
            for idx in sorted(d.ifs):
                i, s = d.ifs[idx], {}
                if "cardinality" in g:
                    s["cardinality"] = {CARDS[q]: len(i.card[q]) for q in range(0 if "conversations" in g else 1, len(CARDS))}
                for t, (dr, metric) in enumerate(TYPES):
                    if "by_" + metric not in g:
                        continue
                    if "counters" in g:
                        for q, kind in enumerate(KINDS):
                            s[f"{dr}_{kind}{metric}"] = i.counters[t][q]
                    for q, top in enumerate(TOPS):
                        if TOP_GROUP[q] in g:
                            s[f"top_{dr}_{top}_{metric}"] = self._top(i.top[t][q])
                for q, metric in enumerate(("bytes", "packets")):
                    if "by_" + metric not in g:
                        continue
                    if "top_geo" in g:
                        # FlowStreamHandler.cpp:1186-1216: written whatever they hold; nothing updates them
                        # without a database (_process_geo_metrics :1453-1497)
                        s["top_geo_loc_" + metric] = []
                        s["top_asn_" + metric] = []
                    if "conversations" in g:
                        s["top_conversations_" + metric] = self._top(i.conv[q])
                if s:
                    ifs[str(idx)] = s
            if ifs:
                ds["interfaces"] = ifs
            if ds:
                devs[name] = ds
        if devs:
            out["devices"] = devs
        return out
