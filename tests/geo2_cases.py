"""The Net v2 geo model (no GPU): a synthetic capture scheduled so that, in every direction, remote
i is counted exactly 3 * 2^i times, and what top_geo_loc_packets / top_asn_packets must then hold
per direction (NetworkMetricsBucket::process_net_layer, net/v2/NetStreamHandler.cpp:494-531,
697-746: in counts the source, out the destination, unknown both), looked up through the
independent reader of tests/mmdb_ref.py. Built on tests/test_gpu_geo_counts.py's frame / record
(its packets() is not used: its unknown-direction packets are not scheduled for distinct counts)."""
import ipaddress
import struct

from tests import mmdb_ref as R
from tests.test_gpu_geo_counts import CITY, HOST, ISP, T0, frame, pcap_of, record  # noqa: F401

DIRS = ("in", "out", "unknown")
# nine of tests/test_gpu_geo_counts.REMOTES (3 * (2^9 - 1) = 1533 counts a direction, about 4600 packets)
REMOTES2 = ["89.160.20.112", "216.160.83.56", "8.8.8.8", "1.128.0.0", "12.81.92.0", "6.6.6.6",
            "2a02:dac0::", "2001:1700::", "2001:db8::77"]
OUTSIDE = {4: "203.0.113.9", 6: "2001:db8::1"}  # the fixed outside address of a family (not in HOST)
LOCAL = {4: "192.168.0.7", 6: "fd00:aaaa::5"}
# unknown direction, remote_i -> remote_j of one family (both counted), and one self pair
PAIRS = [(1, 2), (3, 4), (6, 7), (8, 6)]
SELF = 0


def _ver(a):
    return ipaddress.ip_address(a).version


def packets2(t0=T0, step_us=20, remotes=REMOTES2):
    """[(sec, usec, frame, v1 remote or None, [(direction, counted address), ...])]"""
    plan = []  # (sort key, src, dst, v1 remote, counted)
    for i, rem in enumerate(remotes):
        host = LOCAL[_ver(rem)]
        for k in range(3 << i):
            plan.append(((k, i, 0), rem, host, rem, [("in", rem)]))
            plan.append(((k, i, 1), host, rem, rem, [("out", rem)]))
    left = [3 << i for i in range(len(remotes))]
    plan.append(((0, SELF, 2), remotes[SELF], remotes[SELF], None, [("unknown", remotes[SELF])] * 2))
    left[SELF] -= 2
    for n, (i, j) in enumerate(PAIRS):
        assert _ver(remotes[i]) == _ver(remotes[j])
        plan.append(((1 + n, i, 2), remotes[i], remotes[j], None, [("unknown", remotes[i]), ("unknown", remotes[j])]))
        left[i] -= 1
        left[j] -= 1
    for i, rem in enumerate(remotes):
        assert left[i] > 0
        out = OUTSIDE[_ver(rem)]
        for k in range(left[i]):
            # every other one the other way round: the remote is the destination
            src, dst = (rem, out) if k % 2 == 0 else (out, rem)
            plan.append(((k, i, 3), src, dst, None, [("unknown", src), ("unknown", dst)]))
    plan.sort(key=lambda t: t[0])
    pk, us = [], 0
    for _, src, dst, rem, counted in plan:
        pk.append((t0 + us // 1000000, us % 1000000, frame(src, dst), rem, counted))
        us += step_us
    return pk


def v1_view(pk):
    """the packets as tests/test_gpu_geo_counts.expected() takes them"""
    return [p[:4] for p in pk]


def counted(pk):
    """{direction: {address: times counted}}"""
    out = {d: {} for d in DIRS}
    for p in pk:
        for d, a in p[4]:
            out[d][a] = out[d].get(a, 0) + 1
    return out


def expected2(pk, readers, kinds=("city", "asn")):
    """{direction: {"top_geo_loc_packets": [...], "top_asn_packets": [...]}} as the JSON lists them"""
    cnt = counted(pk)
    out = {}
    for d in DIRS:
        out[d] = {"top_geo_loc_packets": [], "top_asn_packets": []}
        for kind in kinds:
            by = {}
            for a, n in cnt[d].items():
                key = R.lookup(readers[kind], kind, ipaddress.ip_address(a).packed)
                by[key] = by.get(key, 0) + n
            items = []
            for (name, lat, lon), n in by.items():
                it = {"name": name, "estimate": n}
                if kind == "city" and lat and lon:
                    it["lat"], it["lon"] = lat, lon
                items.append(it)
            items.sort(key=lambda it: -it["estimate"])
            assert len({it["estimate"] for it in items}) == len(items), f"per-key counts of {d} / {kind} must be distinct"
            out[d]["top_geo_loc_packets" if kind == "city" else "top_asn_packets"] = items
    return out


def readers():
    return {"city": R.Reader(open(CITY, "rb").read()), "asn": R.Reader(open(ISP, "rb").read())}


def passes(rd, p, prefixes, numbers):
    """the Net geo filters' verdict of a packet (_filtering, net/v2/NetStreamHandler.cpp:223-283):
    unknown direction is filtered; else the remote address's strings against the prefix lists"""
    rem = p[3]
    if rem is None:
        return False
    raw = ipaddress.ip_address(rem).packed
    if prefixes is not None and not any(R.lookup(rd["city"], "city", raw)[0].startswith(x) for x in prefixes):
        return False
    if numbers is not None and not any(R.lookup(rd["asn"], "asn", raw)[0].startswith(n + "/") for n in numbers):
        return False
    return True


def without_geo(j):
    """a window JSON without the v1 and the v2 Net geo lists"""
    import copy
    j = copy.deepcopy(j)
    for w in j.values():
        w["packets"].pop("top_geoLoc", None)
        w["packets"].pop("top_ASN", None)
        for d in DIRS:
            if d in w.get("net", {}):
                w["net"][d].pop("top_geo_loc_packets", None)
                w["net"][d].pop("top_asn_packets", None)
    return j


# ---------------------------------------------------------------- the DNS v2 model
# A completed transaction whose *query* carried a family 1 or 2 ECS option counts once under the
# transaction's direction (DnsMetricsBucket::new_dns_transaction, dns/v2/DnsStreamHandler.cpp:1077-1088):
# out = the client inside the host spec, in = the resolver inside it, unknown = neither.
from tests import dns_geo_cases as D  # noqa: E402
from tests.bgp_cases import ACK, PSH, SYN, tcp  # noqa: E402
from tests.dhcp_cases import eth, ipv4  # noqa: E402

XDIRS = ("in", "out", "unknown")
ENDS = {"out": ("192.168.0.7", "10.9.8.7"), "in": ("203.0.113.50", "192.168.0.53"), "unknown": ("203.0.113.50", "10.9.8.7")}
ENDS6 = {"out": ("fd00:aaaa::5", "2001:db8:53::1"), "in": ("2001:db8:77::9", "fd00:aaaa::53"),
         "unknown": ("2001:db8:77::9", "2001:db8:53::1")}
# five of tests/dns_geo_cases.SUBNETS (3 * (2^5 - 1) = 93 transactions a direction)
SUBNETS2 = [D.SUBNETS[0], D.SUBNETS[1], D.SUBNETS[3], D.SUBNETS[6], D.SUBNETS[9]]
GEO2_DNS = ("top_geo_loc_ecs_xacts", "top_asn_ecs_xacts")


def _pair(n, d, name, q_extra=b"", r_extra=b"", six=False, respond=True):
    """[query frame, response frame] of transaction n in direction d (client port 20000 + n)"""
    cl, rs = (ENDS6 if six else ENDS)[d]
    q = frame(cl, rs, 20000 + n, 53, D.message(n & 0xffff, name, q_extra))
    if not respond:
        return [q]
    return [q, frame(rs, cl, 53, 20000 + n, D.message(n & 0xffff, name, r_extra, qr=1))]


def dns2_packets(t0=T0, step_us=20, keep=None, rd=None, tcp_pair=True, extras=True):
    """([(sec, usec, frame, is_query)], [(direction, subnet)] of the counted transactions).
    keep: "city" / "asn": name a query keep.example.com exactly where its subnet looks up to
    "Unknown" in that database (rd: the readers), drop.example.com elsewhere, for the filter
    equivalence with only_qname."""
    frames, counted_x = [], []
    n = 0
    plan = []
    for i, sub in enumerate(SUBNETS2):
        plan += [(k, i, d) for k in range(3 << i) for d in XDIRS]
    plan.sort()
    for k, i, d in plan:
        sub = SUBNETS2[i]
        name = f"q{n % 7}.example.com"
        if keep:
            name = "keep.example.com" if D.lookup(rd, keep, sub)[0] == "Unknown" else "drop.example.com"
        frames += [(f, j == 0) for j, f in enumerate(_pair(n, d, name, D.opt_rr(D.ecs_option(*sub)), six=n % 3 == 2))]
        counted_x.append((d, sub))
        n += 1
    if extras:
        sub = SUBNETS2[0]
        ecs = D.opt_rr(D.ecs_option(*sub))
        nm = "drop.example.com" if keep else "x.example.com"
        # counted nowhere: a query with ECS and no response, a response with ECS whose query had
        # none, a family-3 option
        extra = _pair(n, "out", nm, ecs, respond=False) + _pair(n + 1, "in", nm, b"", ecs) + \
            _pair(n + 2, "unknown", nm, D.opt_rr(D.ecs_option(3, sub[1])))
        isq = [True, True, False, True, False]
        for j, (f, q) in enumerate(zip(extra, isq)):
            frames.insert(5 + 9 * j, (f, q))
        n += 3
    if tcp_pair:
        # one transaction over TCP (direction out): SYN, the query; SYN|ACK, the response
        sub = SUBNETS2[-1]
        nm = "tcp.example.com"
        if keep:
            nm = "keep.example.com" if D.lookup(rd, keep, sub)[0] == "Unknown" else "drop.example.com"
        qm = D.message(77, nm, D.opt_rr(D.ecs_option(*sub)))
        rm = D.message(77, nm, qr=1)
        cl, rs = ENDS["out"]
        seq = [(eth(ipv4(tcp(b"", 41000, 53, 7000, SYN), 6, cl, rs)), False),
               (eth(ipv4(tcp(b"", 53, 41000, 9000, SYN | ACK), 6, rs, cl)), False),
               (eth(ipv4(tcp(struct.pack(">H", len(qm)) + qm, 41000, 53, 7001, PSH | ACK), 6, cl, rs)), True),
               (eth(ipv4(tcp(struct.pack(">H", len(rm)) + rm, 53, 41000, 9001, PSH | ACK), 6, rs, cl)), False)]
        at = len(frames) // 2
        frames[at:at] = seq
        counted_x.append(("out", sub))
    ts = D.stamps(t0, step_us)
    return [(*next(ts), f, q) for f, q in frames], counted_x


def dns2_pcap(pk) -> bytes:
    return struct.pack("<IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, 65535, 1) + b"".join(record(s, u, f) for s, u, f, _ in pk)


def dns2_expected(counted_x, rd, kinds=("city", "asn")):
    """{direction: {"top_geo_loc_ecs_xacts": [...], "top_asn_ecs_xacts": [...]}} as the JSON lists them"""
    out = {}
    for d in XDIRS:
        out[d] = {k: [] for k in GEO2_DNS}
        for kind in kinds:
            by = {}
            for dd, sub in counted_x:
                if dd == d:
                    key = D.lookup(rd, kind, sub)
                    by[key] = by.get(key, 0) + 1
            items = []
            for (name, lat, lon), cnt in by.items():
                it = {"name": name, "estimate": cnt}
                if kind == "city" and lat and lon:
                    it["lat"], it["lon"] = lat, lon
                items.append(it)
            items.sort(key=lambda it: (-it["estimate"], it["name"]))
            assert len({it["estimate"] for it in items}) == len(items), f"per-key counts of {d} / {kind} must be distinct"
            out[d]["top_geo_loc_ecs_xacts" if kind == "city" else "top_asn_ecs_xacts"] = items
    return out


def without_dns2_geo(j):
    import copy
    j = copy.deepcopy(j)
    for w in j.values():
        for d in XDIRS:
            for k in GEO2_DNS:
                w.get("dns", {}).get(d, {}).pop(k, None)
    return j
