"""DNS v1 top_geoLoc_ecs / top_asn_ecs and the geoloc_notfound / asn_notfound filters on attached
GeoIP databases (pv_set_dns_geo, pv_dns_ecs_geo, pv_dns_geo_verdict): the reference's known
answers on ecs.pcap (src/handlers/dns/v1/tests/test_dns_layer.cpp:711-854) and a synthetic capture
against the Python model of tests/dns_geo_cases.py (the reference's address rule, then the
independent reader of tests/mmdb_ref.py)."""
import copy
import json
import os
import subprocess
import sys

import pytest

import pktvisor_amd as pa
from tests import dns_geo_cases as C

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CITY = os.path.join(GOLD, "GeoIP2-City-Test.mmdb")
ISP = os.path.join(GOLD, "GeoIP2-ISP-Test.mmdb")
ECS = os.path.join(GOLD, "ecs.pcap")
ECS_ON = {"enable": ["top_ecs"]}
U5 = [{"name": "Unknown", "estimate": 5}]
TOPS = ("top_geoLoc_ecs", "top_asn_ecs")


@pytest.fixture(scope="module")
def rd():
    return C.readers(CITY, ISP)


@pytest.fixture(scope="module")
def pk():
    return C.packets()


def handlers(n, periods=1, dns_config=None, city=CITY, asn=ISP, **kw):
    return pa.PvHandlers(host_spec=C.HOST, num_periods=periods, topn_count=50, max_records=max(1, n), net_config={},
                         dns_config=dict(ECS_ON, **(dns_config or {})), geo_city_db=city, geo_asn_db=asn, dns_geo=True, **kw)


def run(tmp_path, pcap, dns_config=None, city=CITY, asn=ISP, dns_geo=True, **kw):
    p = tmp_path / "in.pcap"
    p.write_bytes(pcap)
    return pa.pktvisor_reader(str(p), host_spec=C.HOST, periods=1, topn_count=50, net_config={},
                              dns_config=dict(ECS_ON, **(dns_config or {})), geo_city_db=city, geo_asn_db=asn,
                              dns_geo=dns_geo, **kw)


@pytest.fixture(scope="module")
def gpu(tmp_path_factory, pk):
    """the synthetic capture in one batch, both databases, no filter"""
    return run(tmp_path_factory.mktemp("dns_geo"), C.pcap_of(pk))


def by_name(items):
    return {(it["name"], it.get("lat"), it.get("lon")): it["estimate"] for it in items}


# ---------------------------------------------------------------- the reference's known answers
def kat(dns_config=None, city=CITY, asn=ISP):
    return pa.pktvisor_reader(ECS, host_spec="192.168.0.0/24", periods=1, net_config={},
                              dns_config=dict(ECS_ON, **(dns_config or {})), geo_city_db=city, geo_asn_db=asn,
                              dns_geo=True)["1m"]["dns"]


def test_reference_no_filter():
    d = kat()
    w = d["wire_packets"]
    assert (w["events"], w["tcp"], w["udp"], w["ipv4"], w["ipv6"]) == (36, 4, 32, 6, 30)
    assert (w["queries"], w["replies"], w["filtered"], w["query_ecs"]) == (22, 14, 0, 5)
    assert d["cardinality"]["qname"] == 9
    assert d["top_query_ecs"] == [{"name": "2001:470:1f0b:1600::", "estimate": 5}]
    assert d["top_geoLoc_ecs"] == U5 and d["top_asn_ecs"] == U5


@pytest.mark.parametrize("key,top", [("geoloc_notfound", "top_geoLoc_ecs"), ("asn_notfound", "top_asn_ecs")])
def test_reference_notfound_filters(key, top):
    d = kat({key: True})
    w = d["wire_packets"]
    assert (w["events"], w["tcp"], w["udp"], w["ipv4"], w["ipv6"]) == (36, 0, 5, 1, 4)
    assert (w["queries"], w["replies"], w["filtered"], w["query_ecs"]) == (5, 0, 31, 5)
    assert d["cardinality"]["qname"] == 2
    assert d[top] == U5


def test_reference_one_database():
    d = kat(asn=None)
    assert d["top_geoLoc_ecs"] == U5 and d["top_asn_ecs"] == []
    # a filter family whose database is not attached filters every message
    d = kat({"geoloc_notfound": True}, city=None)
    assert d["wire_packets"]["filtered"] == 36 and d["wire_packets"]["events"] == 36
    assert d["top_geoLoc_ecs"] == [] and d["top_asn_ecs"] == [] and d["top_query_ecs"] == []


# ---------------------------------------------------------------- counts against the model
def test_synthetic_counts(tmp_path, rd, pk, gpu):
    want = C.expected(pk, rd)
    d = gpu["1m"]["dns"]
    assert d["top_geoLoc_ecs"] == want["top_geoLoc_ecs"]
    assert d["top_asn_ecs"] == want["top_asn_ecs"]
    # the TCP query is counted; the family-3 option, the response, the ARCOUNT = 0 query and the OPT
    # records without CSUBNET are counted nowhere
    n = len(C.counted(pk))
    assert d["wire_packets"]["query_ecs"] == n and d["wire_packets"]["tcp"] == 1
    assert d["wire_packets"]["events"] == len(pk) - 1 and d["wire_packets"]["filtered"] == 0
    assert d["top_query_ecs"] == C.expected_query_ecs(pk)
    for k in TOPS:
        assert sum(it["estimate"] for it in d[k]) == n == sum(it["estimate"] for it in d["top_query_ecs"])
    # everything outside the two tops equals the run without the switch (which has to run without
    # the databases, so the Net handler's own geo tops are left out too)
    plain = run(tmp_path, C.pcap_of(pk), city=None, asn=None, dns_geo=False)
    assert plain["1m"]["dns"]["top_geoLoc_ecs"] == [] and plain["1m"]["dns"]["top_asn_ecs"] == []
    a, b = copy.deepcopy(gpu), copy.deepcopy(plain)
    for j in (a, b):
        for k in TOPS:
            j["1m"]["dns"].pop(k)
        for k in ("top_geoLoc", "top_ASN"):
            j["1m"]["packets"].pop(k, None)
    assert a == b


def test_one_database_each(tmp_path, rd, pk):
    want = C.expected(pk, rd)
    d = run(tmp_path, C.pcap_of(pk), asn=None)["1m"]["dns"]
    assert d["top_geoLoc_ecs"] == want["top_geoLoc_ecs"] and d["top_asn_ecs"] == []
    d = run(tmp_path, C.pcap_of(pk), city=None)["1m"]["dns"]
    assert d["top_asn_ecs"] == want["top_asn_ecs"] and d["top_geoLoc_ecs"] == []


@pytest.mark.parametrize("rounds", [9, 40], ids=["72_entries", "320_entries"])
def test_many_entries_in_one_batch_and_split(rd, rounds):
    """more than 64 / more than 256 ECS entries in one batch, eight subnets round-robin (at least
    six dictionary ids of each database among any 64 consecutive ones); the same capture over two
    process_host calls gives the same result"""
    subs = [C.SUBNETS[i] for i in (0, 1, 2, 4, 5, 6, 7, 8)]
    pk = [(C.T0, 10 * n, C.ecs_query(n, subs[n % 8], six=n % 3 == 2), subs[n % 8]) for n in range(8 * rounds)]
    for kind in ("city", "asn"):
        assert len({C.lookup(rd, kind, s) for s in subs}) >= 6
    want = C.expected(pk, rd, distinct=False)
    recs = [C.record(fr, s, u) for s, u, fr, _ in pk]
    got = []
    for cut in (len(recs), len(recs) // 3):
        h = handlers(len(recs))
        try:
            h.process_host(b"".join(recs[:cut]))
            if cut < len(recs):
                h.process_host(b"".join(recs[cut:]))
            got.append(h.window_json(0)["dns"])
        finally:
            h.close()
    for d in got:
        for k in TOPS:
            assert by_name(d[k]) == by_name(want[k]), k
        assert d["wire_packets"]["query_ecs"] == len(pk)
    assert got[0] == got[1]


def test_two_periods_in_one_batch_and_merged(rd):
    a, b = C.packets(), C.packets(t0=C.T0 + 61, tcp_port=41001)  # (each set's TCP query on a connection of its own)
    h = handlers(len(a + b), periods=2)
    try:
        h.process_host(C.records(a + b))
        live, prev, merged = (h.bucket_json(h.merge("dns", None, p, merged=m))["dns"]
                              for p, m in ((0, False), (1, False), (2, True)))
    finally:
        h.close()
    want = C.expected(a, rd)
    # (the second set's first query shifts the DNS window: each bucket holds one whole set)
    for d in (live, prev):
        assert d["wire_packets"]["query_ecs"] == len(C.counted(a)) and d["wire_packets"]["tcp"] == 1
        assert d["top_geoLoc_ecs"] == want["top_geoLoc_ecs"] and d["top_asn_ecs"] == want["top_asn_ecs"]
    both = C.expected(a + b, rd)
    assert merged["top_geoLoc_ecs"] == both["top_geoLoc_ecs"] and merged["top_asn_ecs"] == both["top_asn_ecs"]


def test_slot_reuse_starts_from_zero(rd):
    """18 periods over 16 slots: the newest bucket holds only its own queries"""
    h = handlers(64, periods=2)
    try:
        for p in range(18):
            sub = C.SUBNETS[p % len(C.SUBNETS)]
            h.process_host(b"".join(C.record(C.ecs_query(k, sub), C.T0 + 61 * p, k) for k in range(p + 1)))
        live = h.window_json(0)["dns"]
    finally:
        h.close()
    sub = C.SUBNETS[17 % len(C.SUBNETS)]
    assert live["top_asn_ecs"] == [{"name": C.lookup(rd, "asn", sub)[0], "estimate": 18}]
    assert [it["estimate"] for it in live["top_geoLoc_ecs"]] == [18]
    assert live["top_geoLoc_ecs"][0]["name"] == C.lookup(rd, "city", sub)[0]


# ---------------------------------------------------------------- filters
@pytest.mark.parametrize("kw", [{"geoloc_notfound": True}, {"asn_notfound": True},
                                {"geoloc_notfound": True, "asn_notfound": True}], ids=["geoloc", "asn", "both"])
def test_filters_on_the_synthetic_capture(tmp_path, rd, pk, gpu, kw):
    keep = [p for p in pk if C.passes(rd, p[3], **kw)]
    events = len(pk) - 1  # (the SYN is no DNS event)
    assert 0 < len(keep) < events and any(b"tcp" in p[2] for p in keep)
    d = run(tmp_path, C.pcap_of(pk), dns_config=kw)["1m"]["dns"]
    w = d["wire_packets"]
    assert w["events"] == events == gpu["1m"]["dns"]["wire_packets"]["events"]
    assert w["filtered"] == events - len(keep)
    # the passing set is exactly the ECS queries whose lookup is "Unknown"
    assert w["queries"] == len(keep) == w["query_ecs"] and w["replies"] == 0 and w["tcp"] == 1
    assert d["top_query_ecs"] == C.expected_query_ecs(keep)
    want = C.expected(keep, rd)
    assert d["top_geoLoc_ecs"] == want["top_geoLoc_ecs"] and d["top_asn_ecs"] == want["top_asn_ecs"]
    for fam, top in (("geoloc_notfound", "top_geoLoc_ecs"), ("asn_notfound", "top_asn_ecs")):
        if fam in kw:
            assert d[top] == [{"name": "Unknown", "estimate": len(keep)}]


def test_filter_without_its_database_filters_everything(tmp_path, pk):
    d = run(tmp_path, C.pcap_of(pk), dns_config={"asn_notfound": True}, asn=None)["1m"]["dns"]
    assert d["wire_packets"]["filtered"] == d["wire_packets"]["events"] == len(pk) - 1
    assert d["top_geoLoc_ecs"] == [] and d["top_query_ecs"] == []


def test_filters_with_deep_sampling_are_refused():
    """the deep-sampling prescan cannot read the verdict (it runs ahead of the DNS work lists)"""
    with pytest.raises(pa.PvError, match="deep_sample_rate below 100 with DNS geo filters") as e:
        handlers(64, dns_config={"geoloc_notfound": True, "deep_sample_rate": 50})
    assert "(-4)" in str(e.value)
    # counting alone samples like any other deep metric
    h = handlers(64, dns_config={"deep_sample_rate": 50})
    h.close()


# ---------------------------------------------------------------- outputs
def test_prometheus_and_opentelemetry(pk):
    h = handlers(len(pk))
    try:
        h.process_host(C.records(pk))
        prom = h.window_prometheus(0, handlers="dns")
        otlp = h.window_opentelemetry(0, handlers="dns")
    finally:
        h.close()
    assert "# HELP dns_top_geoLoc_ecs Top GeoIP ECS locations\n# TYPE dns_top_geoLoc_ecs gauge\n" in prom
    assert "# HELP dns_top_asn_ecs Top ASNs by ECS\n# TYPE dns_top_asn_ecs gauge\n" in prom
    assert 'dns_top_geoLoc_ecs{geo_loc="EU/Sweden/E/Linköping",lat="58.416700",lon="15.616700"} 3\n' in prom
    assert 'dns_top_asn_ecs{asn="7018"} 48\n' in prom
    for text in (b"dns_top_geoLoc_ecs", b"dns_top_asn_ecs", b"geo_loc", "EU/Sweden/E/Linköping".encode(), b"58.416700",
                 b"1221/Telstra Pty Ltd"):
        assert text in otlp


def test_prometheus_without_the_switch_has_no_geo_tops(pk):
    h = pa.PvHandlers(host_spec=C.HOST, num_periods=1, topn_count=50, max_records=len(pk), net_config={}, dns_config=ECS_ON)
    try:
        h.process_host(C.records(pk))
        prom = h.window_prometheus(0, handlers="dns")
        d = h.window_json(0)["dns"]
    finally:
        h.close()
    assert "dns_top_query_ecs" in prom and "dns_top_geoLoc_ecs" not in prom and "dns_top_asn_ecs" not in prom
    assert d["top_geoLoc_ecs"] == [] and d["top_asn_ecs"] == []


def test_external_buckets_sum(rd, pk):
    hs = [handlers(len(pk)) for _ in range(2)]
    try:
        for h in hs:
            h.process_host(C.records(pk))
        bucket = hs[0].merge("dns", None, 0)
        bucket = hs[1].merge("dns", bucket, 0)
        d = hs[0].bucket_json(bucket)["dns"]
        prom = hs[0].bucket_prometheus(bucket)
    finally:
        for h in hs:
            h.close()
    want = C.expected(pk + pk, rd)
    assert d["top_geoLoc_ecs"] == want["top_geoLoc_ecs"] and d["top_asn_ecs"] == want["top_asn_ecs"]
    assert 'dns_top_asn_ecs{asn="7018"} 96\n' in prom


def test_kernel_timing_of_the_dns_stage(rd, pk):
    """pv_dns_geo_timing: with the kernel-timing switch on, every batch adds the four DNS-stage
    kernels' event times; the results do not change"""
    h = handlers(len(pk), dns_config={"geoloc_notfound": True})
    try:
        assert h.dns_geo_timing() == ({"pv_dns_geo_verdict": 0.0, "pv_dns_kernel": 0.0, "pv_dns_ecs": 0.0, "pv_dns_ecs_geo": 0.0}, 0)
        h.set_kernel_timing(1)
        h.process_host(C.records(pk))
        ms, n = h.dns_geo_timing(reset=True)
        d = h.window_json(0)["dns"]
    finally:
        h.close()
    assert n >= 1 and all(v > 0 for v in ms.values()) and sum(ms.values()) < 1000
    keep = [p for p in pk if C.passes(rd, p[3], geoloc_notfound=True)]
    assert d["top_geoLoc_ecs"] == [{"name": "Unknown", "estimate": len(keep)}]
    assert d["top_asn_ecs"] == C.expected(keep, rd)["top_asn_ecs"]


# ---------------------------------------------------------------- sharded
def test_sharded_run_matches_single_pass(tmp_path, rd, pk, gpu):
    from tests.dist_launch import ROOT, free_port
    p = tmp_path / "in.pcap"
    p.write_bytes(C.pcap_of(pk))
    out = tmp_path / "out.json"
    port = free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        procs.append(subprocess.Popen([sys.executable, "-m", "tests.dns_geo_dist_worker", str(p), str(out), C.HOST, CITY, ISP],
                                      cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    try:
        for q in procs:
            outs.append(q.communicate(timeout=240)[0].decode(errors="replace"))
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
    assert all(q.returncode == 0 for q in procs), "\n".join(o[-2000:] for o in outs)
    got = json.load(open(out))["1m"]["dns"]
    single = gpu["1m"]["dns"]
    want = C.expected(pk, rd)
    assert got["top_geoLoc_ecs"] == want["top_geoLoc_ecs"] == single["top_geoLoc_ecs"]
    assert got["top_asn_ecs"] == want["top_asn_ecs"] == single["top_asn_ecs"]
    assert got["wire_packets"]["query_ecs"] == single["wire_packets"]["query_ecs"]


def test_rccl_window_reduce_with_databases(rd, pk):
    """pv_comm_allreduce_window with the DNS geo arrays listed (world size 1): they go through RCCL
    and leave the one shard unchanged"""
    h = handlers(len(pk))
    try:
        h.process_host(C.records(pk))
        before = h.window_json(0)["dns"]
        n_regions = len(h.window_regions())
        h.comm_init(pa.comm_unique_id(), 1, 0)
        h.comm_allreduce_window()
        after = h.window_json(0)["dns"]
        h.comm_destroy()
    finally:
        h.close()
    # (Net: sum, cpc, two geo arrays; DNS: sum, cpc, two geo arrays)
    assert n_regions >= 8
    want = C.expected(pk, rd)
    assert after["top_geoLoc_ecs"] == before["top_geoLoc_ecs"] == want["top_geoLoc_ecs"]
    assert after["top_asn_ecs"] == before["top_asn_ecs"] == want["top_asn_ecs"]


# ---------------------------------------------------------------- the opt-in guard
def test_without_the_switch_the_refusals_stand():
    def refused(match, **kw):
        with pytest.raises(pa.PvError, match=match) as e:
            pa.PvHandlers(host_spec=C.HOST, num_periods=1, geo_city_db=CITY, geo_asn_db=ISP, **kw)
        assert "(-4)" in str(e.value)
    refused("top_ecs", net_config={}, dns_config={"enable": ["top_ecs"]})
    refused("DNS geoloc_notfound / asn_notfound", net_config={}, dns_config={"geoloc_notfound": True})
    refused("DNS geoloc_notfound / asn_notfound", net_config={}, dns_config={"asn_notfound": True})


def test_with_the_switch_v2_and_dnstap_stay_refused():
    def refused(match, **kw):
        with pytest.raises(pa.PvError, match=match) as e:
            pa.PvHandlers(host_spec=C.HOST, num_periods=1, geo_city_db=CITY, geo_asn_db=ISP, dns_geo=True, **kw)
        assert "(-4)" in str(e.value)
    refused("DNS v2", dns2_config={})
    refused("Net v2", net2_config={})
    h = handlers(64)
    try:
        with pytest.raises(pa.PvError, match="dnstap") as e:
            h.process_dnstap(open(os.path.join(GOLD, "fixture.dnstap"), "rb").read())
        assert "(-4)" in str(e.value)
    finally:
        h.close()
