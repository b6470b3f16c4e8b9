"""DNS v2 top_geo_loc_ecs_xacts / top_asn_ecs_xacts per transaction direction and the handler's
geoloc_notfound / asn_notfound filters on attached GeoIP databases (pv_set_v2_geo): the reference's
known answers on ecs.pcap (dns/v2/tests/test_dns_layer.cpp:682-831, tests/golden/kat_geo_v2.json)
and the synthetic pairs of tests/geo2_cases.py against their model; everything else in the window
stays equal to the oracle's."""
import json
import os

import pytest

import pktvisor_amd as pa
from tests import geo2_cases as G
from tests.test_gpu_geo_counts import CITY, HOST, ISP, record
from tests.test_gpu_parity import GOLD, diff

pytestmark = pytest.mark.gpu

ECS = os.path.join(GOLD, "ecs.pcap")
KAT = json.load(open(os.path.join(GOLD, "kat_geo_v2.json")))["dns_v2"]
ALL = 0x3ff
ALL_NAMES = ["cardinality", "counters", "quantiles", "top_ecs", "top_qtypes", "top_rcodes", "top_size", "top_qnames",
             "top_ports", "xact_times"]
U2 = [{"name": "Unknown", "estimate": 2}]


@pytest.fixture(scope="module")
def readers():
    return G.readers()


@pytest.fixture(scope="module")
def model(readers):
    pk, counted = G.dns2_packets()
    return {"pk": pk, "pcap": G.dns2_pcap(pk), "want": G.dns2_expected(counted, readers), "counted": counted}


def run(tmp_path, pcap, city=CITY, asn=ISP, **cfg):
    p = tmp_path / "in.pcap"
    p.write_bytes(pcap)
    return pa.pktvisor_reader(str(p), host_spec=HOST, periods=1, topn_count=50, geo_city_db=city, geo_asn_db=asn, v2_geo=True,
                              dns2_config={"enable": ALL_NAMES, **cfg})


def geo_of(dns):
    return {d: {k: dns[d][k] for k in G.GEO2_DNS} for d in G.XDIRS}


# ---------------------------------------------------------------- the reference's known answers
def test_reference_top_ecs_known_answers():
    """:682-731"""
    want = KAT["top_ecs"]
    j = pa.pktvisor_reader(ECS, host_spec=KAT["host_spec"], periods=1, dns2_config={"enable": ["top_ecs"]}, geo_city_db=CITY,
                           geo_asn_db=ISP, v2_geo=True)["1m"]["dns"]
    assert j["observed_packets"] == want["events"] == j["deep_sampled_packets"] and j["filtered_packets"] == 0
    u = j["unknown"]
    assert u["ecs_xacts"] == want["unknown_ecs"] and u["xacts"] == want["xacts"] and u["tcp_xacts"] == want["tcp"]
    assert u["top_ecs_xacts"] == [want["top_ecs_xacts_0"]]
    assert u["top_geo_loc_ecs_xacts"] == [want["top_geo_loc_ecs_xacts_0"]] and u["top_asn_ecs_xacts"] == [want["top_asn_ecs_xacts_0"]]


@pytest.mark.parametrize("key", ["geoloc_notfound", "asn_notfound"])
def test_reference_filter_known_answers(key):
    """:733-831"""
    want = KAT[key]
    j = pa.pktvisor_reader(ECS, host_spec=KAT["host_spec"], periods=1, dns2_config={"enable": ["top_ecs"], key: True},
                           geo_city_db=CITY, geo_asn_db=ISP, v2_geo=True)["1m"]["dns"]
    print(json.dumps(j))
    assert j["observed_packets"] == want["events"] and j["filtered_packets"] == want["filtered_packets"]
    u = j["unknown"]
    assert (u["xacts"], u["orphan_responses"], u["udp_xacts"], u["tcp_xacts"], u["ipv6_xacts"], u["ipv4_xacts"], u["ecs_xacts"]) == \
        (want["xacts"], want["orphan"], want["udp"], 0, want["ipv6"], 0, want["ecs"])
    assert u["cardinality"]["qname"] == want["qname_cardinality"]
    assert u["top_ecs_xacts"] == [want["top_ecs_xacts_0"]]
    assert u[want["geo_top"]] == U2


# ---------------------------------------------------------------- the synthetic pairs against the model
def test_model_conditions(model):
    assert len(model["pk"]) <= 6000
    for d in G.XDIRS:
        for k in G.GEO2_DNS:
            assert len(model["want"][d][k]) >= 3


def test_synthetic_pairs_per_direction(oracle, tmp_path, model):
    gpu = run(tmp_path, model["pcap"])
    dns = gpu["1m"]["dns"]
    assert geo_of(dns) == model["want"]
    for d in G.XDIRS:
        n = sum(1 for dd, _ in model["counted"] if dd == d)
        assert dns[d]["ecs_xacts"] == n == sum(it["estimate"] for it in dns[d]["top_asn_ecs_xacts"])
    assert dns["out"]["tcp_xacts"] == 1
    ref = oracle.run_bytes(model["pcap"], host_spec=HOST, num_periods=1, window=1, topn_count=50, dns2_groups=ALL)
    g, r = G.without_geo(G.without_dns2_geo(gpu)), G.without_geo(G.without_dns2_geo(ref))
    assert diff(g, r) is None, diff(g, r)


def test_every_query_in_the_first_call_every_response_in_the_second(readers):
    """the carried path: the queries' subnets travel with the carried list (the UDP pairs: a TCP
    flow cut between its two directions is a reassembly case of its own)"""
    pk, counted = G.dns2_packets(tcp_pair=False)
    want = G.dns2_expected(counted, readers)
    q = b"".join(record(s, u, f) for s, u, f, isq in pk if isq)
    r = b"".join(record(s, u, f) for s, u, f, isq in pk if not isq)
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, topn_count=50, max_records=len(pk), geo_city_db=CITY, geo_asn_db=ISP,
                      v2_geo=True, dns2_config={"enable": ALL_NAMES})
    try:
        h.process_host(q)
        h.process_host(r)
        dns = h.window_json(0)["dns"]
    finally:
        h.close()
    assert geo_of(dns) == want
    for d in G.XDIRS:
        assert dns[d]["ecs_xacts"] == sum(it["estimate"] for it in dns[d]["top_asn_ecs_xacts"]) == len(counted) // 3


@pytest.mark.parametrize("key,kind", [("geoloc_notfound", "city"), ("asn_notfound", "asn")])
def test_filter_equals_only_qname_on_the_keep_capture(oracle, tmp_path, readers, key, kind):
    """exactly the queries whose subnet looks up to "Unknown" are named keep.example.com
    (tests/test_geo2_model.py checks that premise): both are query-branch filters with one outcome"""
    pk, counted = G.dns2_packets(keep=kind, rd=readers)
    pcap = G.dns2_pcap(pk)
    gpu = run(tmp_path, pcap, **{key: True})
    ref = oracle.run_bytes(pcap, host_spec=HOST, num_periods=1, window=1, topn_count=50, dns2_groups=ALL,
                           only_qname="keep.example.com")
    assert gpu["1m"]["dns"]["filtered_packets"] > 0
    g, r = G.without_geo(G.without_dns2_geo(gpu)), G.without_geo(G.without_dns2_geo(ref))
    assert diff(g["1m"]["dns"], r["1m"]["dns"]) is None, diff(g["1m"]["dns"], r["1m"]["dns"])
    # the geo top of the filter's family then holds "Unknown" alone
    top = "top_geo_loc_ecs_xacts" if kind == "city" else "top_asn_ecs_xacts"
    for d in G.XDIRS:
        assert [it["name"] for it in gpu["1m"]["dns"][d][top]] == ["Unknown"]


def test_only_one_database(tmp_path, model, readers):
    gpu = run(tmp_path, model["pcap"], city=None)
    for d in G.XDIRS:
        assert gpu["1m"]["dns"][d]["top_asn_ecs_xacts"] == model["want"][d]["top_asn_ecs_xacts"]
        assert gpu["1m"]["dns"][d]["top_geo_loc_ecs_xacts"] == []
    # the other family's filter filters every query
    gpu = run(tmp_path, model["pcap"], city=None, geoloc_notfound=True)["1m"]["dns"]
    nq = sum(1 for p in model["pk"] if p[3])
    assert gpu["filtered_packets"] >= nq and all(gpu[d]["top_asn_ecs_xacts"] == [] for d in G.XDIRS if d in gpu)


def test_prometheus_lines(model):
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, topn_count=50, max_records=len(model["pk"]), geo_city_db=CITY, geo_asn_db=ISP,
                      v2_geo=True, dns2_config={"enable": ALL_NAMES})
    try:
        h.process_host(b"".join(record(s, u, f) for s, u, f, _ in model["pk"]))
        prom = h.window_prometheus(0, handlers="dns")
        otlp = h.window_opentelemetry(0, handlers="dns")
    finally:
        h.close()
    assert "# HELP dns_top_geo_loc_ecs_xacts Top GeoIP ECS locations\n# TYPE dns_top_geo_loc_ecs_xacts gauge\n" in prom
    assert "# HELP dns_top_asn_ecs_xacts Top ASNs by ECS\n# TYPE dns_top_asn_ecs_xacts gauge\n" in prom
    for d in G.XDIRS:
        assert f'dns_top_geo_loc_ecs_xacts{{direction="{d}",geo_loc="EU/Sweden/E/Linköping",lat="58.416700",lon="15.616700"}} 3\n' in prom
        assert f'dns_top_asn_ecs_xacts{{asn="1221/Telstra Pty Ltd",direction="{d}"}} 6\n' in prom
    for text in (b"dns_top_geo_loc_ecs_xacts", b"dns_top_asn_ecs_xacts", b"58.416700", b"1221/Telstra Pty Ltd"):
        assert text in otlp


def test_refusals():
    def refused(match, **kw):
        with pytest.raises(pa.PvError, match=match) as e:
            pa.PvHandlers(host_spec=HOST, num_periods=1, geo_city_db=CITY, geo_asn_db=ISP, **kw)
        assert "(-4)" in str(e.value)
    refused("DNS v2", dns2_config={})  # without the switch, as it always was
    refused("DNS v2 geo filters", v2_geo=True, dns2_config={"geoloc_notfound": True, "deep_sample_rate": 50})
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, geo_city_db=CITY, v2_geo=True, dns2_config={})
    try:
        with pytest.raises(pa.PvError, match="dnstap") as e:
            h.process_dnstap(open(os.path.join(GOLD, "fixture.dnstap"), "rb").read())
        assert "(-4)" in str(e.value)
    finally:
        h.close()
