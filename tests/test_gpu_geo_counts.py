"""Net v1 top_geoLoc / top_ASN from attached GeoIP databases (pv_set_geodb, pv_geo_count):
the reference's test databases and known addresses, counted per (direction, address) as
NetworkMetricsBucket::_process_geo_metrics does (net/v1/NetStreamHandler.cpp:745-794), against a
Python count through the independent reader of tests/mmdb_ref.py; everything else in the window
stays equal to the oracle's."""
import copy
import ipaddress
import os
import struct

import pytest

import pktvisor_amd as pa
from tests import mmdb_ref as R
from tests.test_gpu_parity import GOLD, diff

pytestmark = pytest.mark.gpu

CITY = os.path.join(GOLD, "GeoIP2-City-Test.mmdb")
ISP = os.path.join(GOLD, "GeoIP2-ISP-Test.mmdb")
HOST = "192.168.0.0/24,fd00:aaaa::/64"
T0 = 1700000000

# the known addresses of tests/golden/kat_geo.json and some neither database holds
REMOTES = ["89.160.20.112", "216.160.83.56", "81.2.69.142", "8.8.8.8", "1.128.0.0", "6.6.6.6", "12.81.92.0",
           "2a02:dac0::", "2001:218::", "2001:1700::", "2001:db8::77"]


def frame(src: str, dst: str, sport=40000, dport=50000, payload=b"x" * 18) -> bytes:
    """Ethernet + IPv4 / IPv6 + UDP"""
    s, d = ipaddress.ip_address(src), ipaddress.ip_address(dst)
    udp = struct.pack(">HHHH", sport, dport, 8 + len(payload), 0) + payload
    if s.version == 4:
        ip = struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(udp), 0, 0, 64, 17, 0) + s.packed + d.packed
        et = 0x0800
    else:
        ip = struct.pack(">IHBB", 6 << 28, len(udp), 17, 64) + s.packed + d.packed
        et = 0x86DD
    return b"\x02\x00\x00\x00\x00\x01\x02\x00\x00\x00\x00\x02" + struct.pack(">H", et) + ip + udp


def record(sec: int, usec: int, fr: bytes) -> bytes:
    return struct.pack("<IIII", sec, usec, len(fr), len(fr)) + fr


def packets(scale=1, t0=T0, step_us=20):
    """[(sec, usec, frame, counted remote or None)]: remote i sends / receives 3 * 2^i * scale packets,
    alternating directions; every 5th slot adds a packet of unknown direction (counted nowhere)"""
    out = []
    seq = []
    for i, rem in enumerate(REMOTES):
        seq += [(rem, k) for k in range(3 * (1 << i) * scale)]
    # interleave the addresses deterministically
    seq.sort(key=lambda t: (t[1], t[0]))
    us = 0
    for n, (rem, k) in enumerate(seq):
        v6 = ":" in rem
        host = "fd00:aaaa::5" if v6 else "192.168.0.7"
        fr = frame(rem, host) if k % 2 == 0 else frame(host, rem)
        out.append((t0 + us // 1000000, us % 1000000, fr, rem))
        us += step_us
        if n % 5 == 0:
            other = "2001:db8::1" if v6 else "203.0.113.9"
            out.append((t0 + us // 1000000, us % 1000000, frame(rem, other), None))
            us += step_us
    return out


def pcap_of(pk) -> bytes:
    return struct.pack("<IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, 65535, 1) + b"".join(record(s, u, f) for s, u, f, _ in pk)


@pytest.fixture(scope="module")
def readers():
    return {"city": R.Reader(open(CITY, "rb").read()), "asn": R.Reader(open(ISP, "rb").read())}


def expected(pk, readers, kinds=("city", "asn")):
    """{'top_geoLoc': [...], 'top_ASN': [...]} as the JSON lists them (estimate descending)"""
    out = {"top_geoLoc": [], "top_ASN": []}
    for kind in kinds:
        cnt = {}
        for _, _, _, rem in pk:
            if rem is None:
                continue
            key = R.lookup(readers[kind], kind, ipaddress.ip_address(rem).packed)
            cnt[key] = cnt.get(key, 0) + 1
        items = []
        for (name, lat, lon), n in cnt.items():
            it = {"name": name, "estimate": n}
            if kind == "city" and lat and lon:
                it["lat"], it["lon"] = lat, lon
            items.append(it)
        items.sort(key=lambda it: -it["estimate"])
        assert len({it["estimate"] for it in items}) == len(items), "per-key counts must be distinct"
        out["top_geoLoc" if kind == "city" else "top_ASN"] = items
    return out


def without_geo(j):
    j = copy.deepcopy(j)
    for w in j.values():
        w["packets"].pop("top_geoLoc", None)
        w["packets"].pop("top_ASN", None)
    return j


def run(tmp_path, pcap, periods=1, **kw):
    p = tmp_path / "in.pcap"
    p.write_bytes(pcap)
    return pa.pktvisor_reader(str(p), host_spec=HOST, periods=periods, topn_count=50, **kw)


def test_reference_capture_all_unknown(tmp_path):
    """dns_udp_mixed_rcode.pcap (net/v1/tests/test_net_layer.cpp:461-559): no remote address is in
    the test databases, so both tops are the one key "Unknown" with the 24 packets"""
    path = os.path.join(GOLD, "dns_udp_mixed_rcode.pcap")
    j = pa.pktvisor_reader(path, host_spec="192.168.0.0/24", periods=1, geo_city_db=CITY, geo_asn_db=ISP)["1m"]["packets"]
    assert j["top_ipv4"][0] == {"name": "198.51.44.1", "estimate": 4}
    assert j["top_geoLoc"] == [{"name": "Unknown", "estimate": 24}]
    assert j["top_ASN"] == [{"name": "Unknown", "estimate": 24}]
    assert j["filtered"] == 0
    j = pa.pktvisor_reader(path, host_spec="192.168.0.0/24", periods=1, geo_city_db=CITY)["1m"]["packets"]
    assert j["top_geoLoc"] == [{"name": "Unknown", "estimate": 24}] and j["top_ASN"] == []
    j = pa.pktvisor_reader(path, host_spec="192.168.0.0/24", periods=1)["1m"]["packets"]
    assert j["top_geoLoc"] == [] and j["top_ASN"] == []


@pytest.mark.parametrize("net_config", [None, {"disable": ["cardinality"]}], ids=["default", "no_cardinality"])
def test_synthetic_capture_counts(oracle, tmp_path, readers, net_config):
    pk = packets()
    pcap = pcap_of(pk)
    kw = {"net_config": net_config, "dns_config": {}} if net_config else {}
    gpu = run(tmp_path, pcap, geo_city_db=CITY, geo_asn_db=ISP, **kw)
    want = expected(pk, readers)
    got = gpu["1m"]["packets"]
    assert got["top_geoLoc"] == want["top_geoLoc"]
    assert got["top_ASN"] == want["top_ASN"]
    names = [it["name"] for it in got["top_ASN"]]
    assert "" in names and "Unknown" in names and "7018" in names  # the empty string is a key of its own
    assert {"name": "EU/Sweden/E/Linköping", "estimate": 3, "lat": "58.416700", "lon": "15.616700"} in got["top_geoLoc"]
    # each geo top counts exactly what top_ipv4 + top_ipv6 count
    ips = sum(it["estimate"] for it in got["top_ipv4"] + got["top_ipv6"])
    assert ips == sum(1 for p in pk if p[3]) > 6000
    assert sum(it["estimate"] for it in got["top_geoLoc"]) == ips == sum(it["estimate"] for it in got["top_ASN"])
    # the rest of the window is the oracle's
    okw = {"net_groups": pa.PV_NET_COUNTERS | pa.PV_NET_TOP_GEO | pa.PV_NET_TOP_IPS} if net_config else {}
    ref = oracle.run_bytes(pcap, host_spec=HOST, num_periods=1, window=1, topn_count=50, **okw)
    assert diff(without_geo(gpu), without_geo(ref)) is None, diff(without_geo(gpu), without_geo(ref))


def test_two_process_host_calls(tmp_path, readers):
    pk = packets()
    recs = [record(s, u, f) for s, u, f, _ in pk]
    cut = len(recs) // 3
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, topn_count=50, max_records=len(recs), geo_city_db=CITY, geo_asn_db=ISP)
    try:
        h.process_host(b"".join(recs[:cut]))
        h.process_host(b"".join(recs[cut:]))
        got = h.window_json(0)["packets"]
    finally:
        h.close()
    want = expected(pk, readers)
    assert got["top_geoLoc"] == want["top_geoLoc"] and got["top_ASN"] == want["top_ASN"]


def test_topn_count_and_percentile_apply(tmp_path, readers):
    pk = packets()
    p = tmp_path / "in.pcap"
    p.write_bytes(pcap_of(pk))
    want = expected(pk, readers)
    j = pa.pktvisor_reader(str(p), host_spec=HOST, periods=1, topn_count=3, geo_city_db=CITY, geo_asn_db=ISP)["1m"]["packets"]
    assert j["top_geoLoc"] == want["top_geoLoc"][:3] and j["top_ASN"] == want["top_ASN"][:3]
    j = pa.pktvisor_reader(str(p), host_spec=HOST, periods=1, topn_count=4, topn_percentile_threshold=50,
                           geo_city_db=CITY, geo_asn_db=ISP)["1m"]["packets"]
    assert j["top_ASN"] == want["top_ASN"][:3]  # the 2nd smallest of the 4 leading estimates is the cut


def test_windows_buckets_and_merged(tmp_path, readers):
    a, b = packets(), packets(t0=T0 + 61)
    recs = b"".join(record(s, u, f) for s, u, f, _ in a + b)
    h = pa.PvHandlers(host_spec=HOST, num_periods=2, topn_count=50, max_records=len(a + b), geo_city_db=CITY, geo_asn_db=ISP)
    try:
        h.process_host(recs)
        # (read through the Net handler's buckets: the capture holds no DNS event, so the DNS
        # manager's window never shifts and a window_json of both handlers has no period 1)
        live, prev, merged = (h.bucket_json(h.merge("net", None, p, merged=m))["packets"]
                              for p, m in ((0, False), (1, False), (2, True)))
    finally:
        h.close()
    want = expected(a, readers)
    # (the second period's first packet shifts the window: both buckets hold one whole set)
    assert live["top_ASN"] == want["top_ASN"] and prev["top_ASN"] == want["top_ASN"]
    assert live["top_geoLoc"] == want["top_geoLoc"] and prev["top_geoLoc"] == want["top_geoLoc"]
    both = expected(a + b, readers)
    assert merged["top_ASN"] == both["top_ASN"] and merged["top_geoLoc"] == both["top_geoLoc"]


def test_slot_reuse_starts_from_zero(readers):
    """18 periods over 16 slots: the newest bucket holds only its own packets"""
    h = pa.PvHandlers(host_spec=HOST, num_periods=2, topn_count=50, max_records=64, geo_city_db=CITY, geo_asn_db=ISP)
    try:
        for p in range(18):
            rem = REMOTES[p % len(REMOTES)]
            fr = frame(rem, "fd00:aaaa::5" if ":" in rem else "192.168.0.7")
            h.process_host(b"".join(record(T0 + 61 * p, k, fr) for k in range(p + 1)))
        live = h.window_json(0)["packets"]
    finally:
        h.close()
    rem = ipaddress.ip_address(REMOTES[17 % len(REMOTES)]).packed
    assert live["top_ASN"] == [{"name": R.lookup(readers["asn"], "asn", rem)[0], "estimate": 18}]
    assert [it["estimate"] for it in live["top_geoLoc"]] == [18]


def test_external_buckets_sum(readers):
    pk = packets()
    recs = b"".join(record(s, u, f) for s, u, f, _ in pk)
    hs = [pa.PvHandlers(host_spec=HOST, num_periods=1, topn_count=50, max_records=len(pk), geo_city_db=CITY, geo_asn_db=ISP)
          for _ in range(2)]
    try:
        for h in hs:
            h.process_host(recs)
        bucket = hs[0].merge("net", None, 0)
        bucket = hs[1].merge("net", bucket, 0)
        j = hs[0].bucket_json(bucket)["packets"]
        prom = hs[0].bucket_prometheus(bucket)
    finally:
        for h in hs:
            h.close()
    want = expected(pk + pk, readers)
    assert j["top_geoLoc"] == want["top_geoLoc"] and j["top_ASN"] == want["top_ASN"]
    assert 'packets_top_ASN{asn="1221/Telstra Pty Ltd"} 96' in prom


def test_prometheus_and_opentelemetry(readers):
    pk = packets()
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, topn_count=50, max_records=len(pk), geo_city_db=CITY, geo_asn_db=ISP)
    try:
        h.process_host(b"".join(record(s, u, f) for s, u, f, _ in pk))
        prom = h.window_prometheus(0, handlers="net")
        otlp = h.window_opentelemetry(0, handlers="net")
    finally:
        h.close()
    assert "# HELP packets_top_geoLoc Top GeoIP locations\n# TYPE packets_top_geoLoc gauge\n" in prom
    assert "# HELP packets_top_ASN Top ASNs by IP\n# TYPE packets_top_ASN gauge\n" in prom
    assert 'packets_top_geoLoc{geo_loc="EU/Sweden/E/Linköping",lat="58.416700",lon="15.616700"} 3\n' in prom
    assert 'packets_top_geoLoc{geo_loc="EU/Russia",lat="60.000000",lon="100.000000"} 384\n' in prom
    assert 'packets_top_ASN{asn="7018"} 192\n' in prom and 'packets_top_ASN{asn=""} 24\n' in prom
    for text in (b"packets_top_geoLoc", b"packets_top_ASN", b"geo_loc", "EU/Sweden/E/Linköping".encode(), b"58.416700",
                 b"1221/Telstra Pty Ltd"):
        assert text in otlp


def test_refusals():
    def refused(msg, **kw):
        with pytest.raises(pa.PvError, match=msg) as e:
            pa.PvHandlers(host_spec=HOST, num_periods=1, geo_city_db=CITY, **kw)
        assert "(-4)" in str(e.value)
    refused("Net v2", net2_config={})
    refused("DNS v2", dns2_config={})
    refused("top_ecs", net_config={}, dns_config={"enable": ["top_ecs"]})
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, geo_city_db=CITY)
    try:
        with pytest.raises(pa.PvError, match="dnstap") as e:
            h.process_dnstap(open(os.path.join(GOLD, "fixture.dnstap"), "rb").read())
        assert "(-4)" in str(e.value)
    finally:
        h.close()


def _run_geo_ranks(world, args, timeout=240):
    """tests/dist_launch.run_ranks for tests/geo_dist_worker.py"""
    import subprocess
    import sys
    from tests.dist_launch import ROOT, free_port
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        procs.append(subprocess.Popen([sys.executable, "-m", "tests.geo_dist_worker", *args], cwd=ROOT, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0].decode(errors="replace"))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return [(p.returncode, o) for p, o in zip(procs, outs)]


def test_sharded_run_matches_single_pass(tmp_path, readers):
    import json
    pk = packets()
    p = tmp_path / "in.pcap"
    p.write_bytes(pcap_of(pk))
    out = tmp_path / "out.json"
    res = _run_geo_ranks(2, [str(p), str(out), HOST, CITY, ISP])
    assert all(rc == 0 for rc, _ in res), "\n".join(o[-2000:] for _, o in res)
    got = json.load(open(out))["1m"]["packets"]
    single = run(tmp_path, pcap_of(pk), geo_city_db=CITY, geo_asn_db=ISP)["1m"]["packets"]
    want = expected(pk, readers)
    assert got["top_geoLoc"] == want["top_geoLoc"] == single["top_geoLoc"]
    assert got["top_ASN"] == want["top_ASN"] == single["top_ASN"]
    assert got["total"] == single["total"]


def test_sharded_run_refuses_different_databases(tmp_path):
    from tests import geo_cases
    p = tmp_path / "in.pcap"
    p.write_bytes(pcap_of(packets()))
    other = tmp_path / "other.mmdb"
    other.write_bytes(R.write_mmdb(geo_cases.V4, 24, 4))
    res = _run_geo_ranks(2, [str(p), str(tmp_path / "out.json"), HOST, CITY, ISP, str(other)])
    assert all(rc != 0 for rc, _ in res)
    assert any("geo databases differ across ranks" in o for _, o in res), "\n".join(o[-1500:] for _, o in res)
    assert not (tmp_path / "out.json").exists()


# ---------------------------------------------------------------- geo filters on the databases
MIXED = os.path.join(GOLD, "dns_udp_mixed_rcode.pcap")
U24 = [{"name": "Unknown", "estimate": 24}]


@pytest.mark.parametrize("net_config,city,asn,want", [
    ({"geoloc_notfound": True}, CITY, ISP, {"top_geoLoc": U24, "filtered": 0, "top4": True}),
    ({"asn_notfound": True}, CITY, ISP, {"top_ASN": U24, "filtered": 0, "top4": True}),
    ({"geoloc_notfound": True, "asn_notfound": True}, CITY, ISP, {"top_geoLoc": U24, "top_ASN": U24, "filtered": 0, "top4": True}),
    ({"only_geoloc_prefix": ["NA/United States"]}, CITY, ISP, {"top_geoLoc": [], "filtered": 24}),
    ({"only_asn_number": ["16509", "22131"]}, CITY, ISP, {"top_ASN": [], "filtered": 24}),
    ({"asn_notfound": True}, CITY, None, {"top_ASN": [], "top_geoLoc": [], "filtered": 24}),
], ids=["geoloc_notfound", "asn_notfound", "both", "only_geoloc_prefix", "only_asn_number", "city_only_asn_notfound"])
def test_reference_filter_known_answers(net_config, city, asn, want):
    """net/v1/tests/test_net_layer.cpp:461-559 on dns_udp_mixed_rcode.pcap, host 192.168.0.0/24"""
    j = pa.pktvisor_reader(MIXED, host_spec="192.168.0.0/24", periods=1, net_config=net_config, dns_config={},
                           geo_city_db=city, geo_asn_db=asn)["1m"]["packets"]
    assert j["events"] == 24 and j["filtered"] == want["filtered"]
    for k in ("top_geoLoc", "top_ASN"):
        if k in want:
            assert j[k] == want[k], k
    if want.get("top4"):
        assert j["top_ipv4"][0] == {"name": "198.51.44.1", "estimate": 4}
    else:
        assert j["top_ipv4"] == [] and j["total"] == 0


def _bracketed(rem):
    """the synthetic capture with one packet of `rem` before and after it (so the first and the
    last packet pass a filter that passes `rem`: the period's bounds are then the oracle's)"""
    host = "fd00:aaaa::5" if ":" in rem else "192.168.0.7"
    return [(T0, 0, frame(rem, host), rem)] + packets(t0=T0 + 1) + [(T0 + 3, 0, frame(host, rem), rem)]


def _passes(readers, rem, prefixes, numbers):
    if rem is None:
        return False  # unknown direction
    raw = ipaddress.ip_address(rem).packed
    if prefixes is not None and not any(R.lookup(readers["city"], "city", raw)[0].startswith(p) for p in prefixes):
        return False
    if numbers is not None and not any(R.lookup(readers["asn"], "asn", raw)[0].startswith(n + "/") for n in numbers):
        return False
    return True


@pytest.mark.parametrize("prefixes,numbers,anchor,passing", [
    (["EU/"], None, "89.160.20.112", {"89.160.20.112", "81.2.69.142", "2a02:dac0::"}),
    (None, ["1221", "7018"], "1.128.0.0", {"1.128.0.0"}),           # "7018" has no slash: 12.81.92.0 is filtered
    (["EU/"], ["29518", "7018"], "89.160.20.112", {"89.160.20.112"}),  # the two families are and-ed
], ids=["geoloc_prefix", "asn_number", "both"])
def test_filters_on_the_synthetic_capture(oracle, tmp_path, readers, prefixes, numbers, anchor, passing):
    pk = _bracketed(anchor)
    keep = [p for p in pk if _passes(readers, p[3], prefixes, numbers)]
    assert {p[3] for p in keep} == passing and "12.81.92.0" not in passing
    cfg = {}
    if prefixes is not None:
        cfg["only_geoloc_prefix"] = prefixes
    if numbers is not None:
        cfg["only_asn_number"] = numbers
    gpu = run(tmp_path, pcap_of(pk), net_config=cfg, dns_config={}, geo_city_db=CITY, geo_asn_db=ISP)
    ref = oracle.run_bytes(pcap_of(keep), host_spec=HOST, num_periods=1, window=1, topn_count=50)
    nf = len(pk) - len(keep)
    ref["1m"]["packets"]["events"] += nf
    ref["1m"]["packets"]["deep_samples"] += nf
    ref["1m"]["packets"]["filtered"] = nf
    assert diff(without_geo(gpu), without_geo(ref)) is None, diff(without_geo(gpu), without_geo(ref))
    want = expected(keep, readers)
    assert gpu["1m"]["packets"]["top_geoLoc"] == want["top_geoLoc"] and gpu["1m"]["packets"]["top_ASN"] == want["top_ASN"]


def test_issue_filter_pair_filters_everything(tmp_path, readers):
    """only_geoloc_prefix [EU/] and only_asn_number [1221, 7018] together: no address of the
    capture is in Europe and in one of those networks ("7018" without an organisation matches
    nothing), so every packet is a filtered event"""
    pk = packets()
    assert not [p for p in pk if _passes(readers, p[3], ["EU/"], ["1221", "7018"])]
    j = run(tmp_path, pcap_of(pk), net_config={"only_geoloc_prefix": ["EU/"], "only_asn_number": ["1221", "7018"]},
            dns_config={}, geo_city_db=CITY, geo_asn_db=ISP)["1m"]["packets"]
    assert j["events"] == j["filtered"] == j["deep_samples"] == len(pk) and j["total"] == 0
    assert j["top_geoLoc"] == [] and j["top_ASN"] == [] and j["top_ipv4"] == [] and j["top_ipv6"] == []


@pytest.mark.parametrize("disable", [["top_ips"], ["top_ips", "cardinality"]], ids=["no_top_ips", "no_top_ips_no_cardinality"])
def test_counts_with_top_ips_disabled(oracle, tmp_path, readers, disable):
    pk = packets()
    gpu = run(tmp_path, pcap_of(pk), net_config={"disable": disable}, dns_config={}, geo_city_db=CITY, geo_asn_db=ISP)
    got, want = gpu["1m"]["packets"], expected(pk, readers)
    assert got["top_geoLoc"] == want["top_geoLoc"] and got["top_ASN"] == want["top_ASN"]
    assert "top_ipv4" not in got and "top_ipv6" not in got
    groups = pa.PV_NET_COUNTERS | pa.PV_NET_TOP_GEO | (0 if "cardinality" in disable else pa.PV_NET_CARDINALITY)
    ref = oracle.run_bytes(pcap_of(pk), host_spec=HOST, num_periods=1, window=1, topn_count=50, net_groups=groups)
    assert diff(without_geo(gpu), without_geo(ref)) is None, diff(without_geo(gpu), without_geo(ref))


def test_filter_and_dns_refusals():
    def refused(match, **kw):
        with pytest.raises(pa.PvError, match=match) as e:
            pa.PvHandlers(host_spec=HOST, num_periods=1, geo_city_db=CITY, geo_asn_db=ISP, **kw)
        assert "(-4)" in str(e.value)
    # the DNS handler's geo filters are not built on a database
    refused("DNS geoloc_notfound / asn_notfound", net_config={}, dns_config={"geoloc_notfound": True})
    refused("DNS geoloc_notfound / asn_notfound", net_config={}, dns_config={"asn_notfound": True})
    # sampling with a Net geo filter stays refused, database or not
    refused("geo filters", net_config={"geoloc_notfound": True, "deep_sample_rate": 50}, dns_config={})
    with pytest.raises(pa.PvError, match="geo filters"):
        pa.PvHandlers(host_spec=HOST, num_periods=1, net_config={"geoloc_notfound": True, "deep_sample_rate": 50}, dns_config={})
    # a non-digit ASN number through the C ABI carries the reference's text
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, geo_city_db=CITY, geo_asn_db=ISP)
    try:
        with pytest.raises(pa.PvError, match="only_asn_number filter contained an invalid/unsupported value: 16509/Amazon"):
            h.set_net_filters(only_asn_number=["16509/Amazon"])
    finally:
        h.close()


def test_names_with_separator_bytes_are_not_geo_items(oracle, tmp_path):
    """a query name whose labels hold 0x1f bytes (the byte the geo items' triple is joined with
    inside a bucket) renders as every other name does, with or without a database attached"""
    def query(txid, labels):
        q = b"".join(bytes([len(l)]) + l for l in labels) + b"\x00"
        return struct.pack(">HHHHHH", txid, 0x0100, 1, 0, 0, 0) + q + struct.pack(">HH", 1, 1)
    pk = []
    for k in range(40):
        labels = [b"a\x1fb\x1fc", b"x\x1f", b"example", b"com"] if k % 2 else [b"\x1f\x1f", b"example", b"org"]
        fr = frame("192.168.0.7", "89.160.20.112", sport=30000 + k, dport=53, payload=query(k, labels))
        pk.append((T0, k * 10, fr, "89.160.20.112"))
    pcap = pcap_of(pk)
    ref = oracle.run_bytes(pcap, host_spec=HOST, num_periods=1, window=1, topn_count=50)
    assert sum(it["name"].count("\x1f") >= 2 for it in ref["1m"]["dns"]["top_qname3"]) >= 1
    gpu = run(tmp_path, pcap)
    assert diff(gpu, ref) is None, diff(gpu, ref)
    gpu = run(tmp_path, pcap, geo_city_db=CITY, geo_asn_db=ISP)
    assert diff(without_geo(gpu), without_geo(ref)) is None
    assert all(set(it) == {"name", "estimate"} for k, v in gpu["1m"]["dns"].items() if k.startswith("top_") for it in v)
    assert gpu["1m"]["packets"]["top_geoLoc"] == [{"name": "EU/Sweden/E/Linköping", "estimate": 40, "lat": "58.416700",
                                                   "lon": "15.616700"}]


def test_rccl_window_reduce_with_databases(readers):
    """pv_comm_allreduce_window with databases attached (world size 1, as tests/test_gpu_rccl.py):
    the hash gather and the geo count regions go through RCCL and leave the one shard unchanged"""
    pk = packets()
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, topn_count=50, max_records=len(pk), geo_city_db=CITY, geo_asn_db=ISP)
    try:
        h.process_host(b"".join(record(s, u, f) for s, u, f, _ in pk))
        before = h.window_json(0)["packets"]
        assert len(h.window_regions()) >= 4 and h.geo_hashes[0] and h.geo_hashes[1] and h.geo_hashes[0] != h.geo_hashes[1]
        h.comm_init(pa.comm_unique_id(), 1, 0)
        h.comm_allreduce_window()
        after = h.window_json(0)["packets"]
        h.comm_destroy()
    finally:
        h.close()
    want = expected(pk, readers)
    assert after["top_geoLoc"] == before["top_geoLoc"] == want["top_geoLoc"]
    assert after["top_ASN"] == before["top_ASN"] == want["top_ASN"]
