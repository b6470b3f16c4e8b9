"""Net v2 top_geo_loc_packets / top_asn_packets per direction and the handler's own geo filters
on attached GeoIP databases (pv_set_v2_geo, pv_set_net2_filters): the reference's known answers
(net/v2/tests/test_net_layer.cpp:453-551, tests/golden/kat_geo_v2.json) and the synthetic capture
of tests/geo2_cases.py against its model, next to Net v1; everything else in the window stays
equal to the oracle's."""
import ipaddress
import json
import os

import pytest

import pktvisor_amd as pa
from tests import geo2_cases as G
from tests import mmdb_ref as R
from tests.test_gpu_geo_counts import CITY, HOST, ISP, REMOTES, T0, expected, frame, pcap_of, record
from tests.test_gpu_parity import GOLD, diff

pytestmark = pytest.mark.gpu

MIXED = os.path.join(GOLD, "dns_udp_mixed_rcode.pcap")
KAT = json.load(open(os.path.join(GOLD, "kat_geo_v2.json")))
GEO = ("top_geo_loc_packets", "top_asn_packets")
N2_ALL = 31  # the oracle's Net v2 group bits


@pytest.fixture(scope="module")
def readers():
    return G.readers()


@pytest.fixture(scope="module")
def model(readers):
    """the synthetic capture, its v2 model and its v1 model, computed once"""
    pk = G.packets2()
    return {"pk": pk, "pcap": pcap_of(G.v1_view(pk)), "v2": G.expected2(pk, readers), "v1": expected(G.v1_view(pk), readers)}


def run(tmp_path, pcap, periods=1, **kw):
    p = tmp_path / "in.pcap"
    p.write_bytes(pcap)
    kw.setdefault("net2_config", {})
    return pa.pktvisor_reader(str(p), host_spec=HOST, periods=periods, topn_count=50, geo_city_db=CITY, geo_asn_db=ISP,
                              v2_geo=True, **kw)


def handlers(n, **kw):
    kw.setdefault("net2_config", {})
    return pa.PvHandlers(host_spec=HOST, topn_count=50, max_records=n, geo_city_db=CITY, geo_asn_db=ISP, v2_geo=True, **kw)


def geo_of(net):
    return {d: {k: net[d][k] for k in GEO} for d in G.DIRS}


# ---------------------------------------------------------------- the reference's known answers
@pytest.mark.parametrize("case", KAT["net_v2"], ids=[c["id"] for c in KAT["net_v2"]])
def test_reference_known_answers(case):
    j = pa.pktvisor_reader(MIXED, host_spec=KAT["host_spec"], periods=1, net2_config=case["config"], geo_city_db=CITY,
                           geo_asn_db=ISP, v2_geo=True)["1m"]
    net = j["net"]
    assert net["observed_packets"] == 24
    if "in" in case:
        assert net["filtered_packets"] == 0
        for key, want in case["in"].items():
            assert net["in"][key[:-2]][0] == want, key
    else:
        assert net["filtered_packets"] == case["filtered_packets"] == net["deep_sampled_packets"]
        # no direction was counted: no geo item anywhere (the reference reads a null name)
        assert not any(d in net for d in G.DIRS)
    # the v1 handler next to it has no filter of its own: it counts every packet
    assert j["packets"]["filtered"] == 0 and j["packets"]["top_geoLoc"] == [{"name": "Unknown", "estimate": 24}]


def test_invalid_asn_number_through_the_c_abi():
    h = handlers(64, num_periods=1)
    try:
        with pytest.raises(pa.PvError, match=KAT["invalid_asn_number"]["error"]):
            h.set_net_filters(v2=True, only_asn_number=[KAT["invalid_asn_number"]["value"]])
    finally:
        h.close()


# ---------------------------------------------------------------- the synthetic capture against the model
@pytest.mark.parametrize("v1_geo", [True, False], ids=["v1_top_geo", "v1_top_geo_disabled"])
def test_synthetic_capture_counts(oracle, tmp_path, model, v1_geo):
    kw = {} if v1_geo else {"net_config": {"disable": ["top_geo"]}, "dns_config": {}}
    gpu = run(tmp_path, model["pcap"], **kw)
    net, v1 = gpu["1m"]["net"], gpu["1m"]["packets"]
    assert geo_of(net) == model["v2"]
    for d in G.DIRS:
        # each geo top counts exactly what the direction's IP tops count
        ips = sum(it["estimate"] for it in net[d]["top_ipv4_packets"] + net[d]["top_ipv6_packets"])
        assert ips == sum(it["estimate"] for it in net[d]["top_geo_loc_packets"]) == sum(it["estimate"] for it in net[d]["top_asn_packets"])
    if v1_geo:
        assert v1["top_geoLoc"] == model["v1"]["top_geoLoc"] and v1["top_ASN"] == model["v1"]["top_ASN"]
    else:
        assert "top_geoLoc" not in v1 and "top_ASN" not in v1
    okw = {} if v1_geo else {"net_groups": pa.PV_NET_COUNTERS | pa.PV_NET_CARDINALITY | pa.PV_NET_TOP_IPS}
    ref = oracle.run_bytes(model["pcap"], host_spec=HOST, num_periods=1, window=1, topn_count=50, net2_groups=N2_ALL, **okw)
    assert diff(G.without_geo(gpu), G.without_geo(ref)) is None, diff(G.without_geo(gpu), G.without_geo(ref))


def test_v2_top_geo_disabled_v1_still_counts(tmp_path, model):
    gpu = run(tmp_path, model["pcap"], net2_config={"disable": ["top_geo"]})
    net, v1 = gpu["1m"]["net"], gpu["1m"]["packets"]
    assert not any(k in net[d] for d in G.DIRS for k in GEO)
    assert v1["top_geoLoc"] == model["v1"]["top_geoLoc"] and v1["top_ASN"] == model["v1"]["top_ASN"]


@pytest.mark.parametrize("disable,groups", [(["top_ips"], 1 | 2 | 4 | 8), (["top_ips", "cardinality"], 1 | 4 | 8)],
                         ids=["no_top_ips", "no_top_ips_no_cardinality"])
def test_counts_with_top_ips_disabled(oracle, tmp_path, model, disable, groups):
    gpu = run(tmp_path, model["pcap"], net2_config={"disable": disable})
    net = gpu["1m"]["net"]
    assert geo_of(net) == model["v2"]
    assert not any(k in net[d] for d in G.DIRS for k in ("top_ipv4_packets", "top_ipv6_packets"))
    ref = oracle.run_bytes(model["pcap"], host_spec=HOST, num_periods=1, window=1, topn_count=50, net2_groups=groups)
    assert diff(G.without_geo(gpu), G.without_geo(ref)) is None, diff(G.without_geo(gpu), G.without_geo(ref))


def test_only_one_database(tmp_path, model, readers):
    p = tmp_path / "in.pcap"
    p.write_bytes(model["pcap"])
    net = pa.pktvisor_reader(str(p), host_spec=HOST, periods=1, topn_count=50, net2_config={}, geo_asn_db=ISP, v2_geo=True)["1m"]["net"]
    for d in G.DIRS:
        assert net[d]["top_asn_packets"] == model["v2"][d]["top_asn_packets"] and net[d]["top_geo_loc_packets"] == []


def test_two_process_host_calls(model):
    recs = [record(s, u, f) for s, u, f, _ in G.v1_view(model["pk"])]
    cut = len(recs) // 3
    h = handlers(len(recs), num_periods=1)
    try:
        h.process_host(b"".join(recs[:cut]))
        h.process_host(b"".join(recs[cut:]))
        got = h.window_json(0)
    finally:
        h.close()
    assert geo_of(got["net"]) == model["v2"]
    assert got["packets"]["top_ASN"] == model["v1"]["top_ASN"]


def test_topn_count_and_percentile_apply(tmp_path, model):
    p = tmp_path / "in.pcap"
    p.write_bytes(model["pcap"])
    kw = dict(host_spec=HOST, periods=1, net2_config={}, geo_city_db=CITY, geo_asn_db=ISP, v2_geo=True)
    net = pa.pktvisor_reader(str(p), topn_count=3, **kw)["1m"]["net"]
    for d in G.DIRS:
        assert net[d]["top_asn_packets"] == model["v2"][d]["top_asn_packets"][:3]
        assert net[d]["top_geo_loc_packets"] == model["v2"][d]["top_geo_loc_packets"][:3]
    net = pa.pktvisor_reader(str(p), topn_count=4, topn_percentile_threshold=50, **kw)["1m"]["net"]
    assert net["unknown"]["top_asn_packets"] == model["v2"]["unknown"]["top_asn_packets"][:3]


def test_windows_buckets_and_merged(readers, model):
    a, b = model["pk"], G.packets2(t0=T0 + 61)
    recs = b"".join(record(s, u, f) for s, u, f, _ in G.v1_view(a + b))
    h = handlers(len(a + b), num_periods=2)
    try:
        h.process_host(recs)
        live, prev, merged = (h.bucket_json(h.merge("net", None, p, merged=m))["net"]
                              for p, m in ((0, False), (1, False), (2, True)))
    finally:
        h.close()
    assert geo_of(live) == model["v2"] and geo_of(prev) == model["v2"]
    assert geo_of(merged) == G.expected2(a + b, readers)


def test_slot_reuse_starts_from_zero(readers):
    """18 periods over 16 slots: the newest bucket holds only its own packets"""
    h = handlers(64, num_periods=2)
    try:
        for p in range(18):
            rem = REMOTES[p % len(REMOTES)]
            local = "fd00:aaaa::5" if ":" in rem else "192.168.0.7"
            # in, out and unknown packets of the period's remote
            frs = [frame(rem, local), frame(local, rem), frame(rem, G.OUTSIDE[6 if ":" in rem else 4])]
            h.process_host(b"".join(record(T0 + 61 * p, k, frs[k % 3]) for k in range(3 * (p + 1))))
        live = h.window_json(0)["net"]
    finally:
        h.close()
    rem = REMOTES[17 % len(REMOTES)]
    name = R.lookup(readers["asn"], "asn", ipaddress.ip_address(rem).packed)[0]
    out = R.lookup(readers["asn"], "asn", ipaddress.ip_address(G.OUTSIDE[6 if ":" in rem else 4]).packed)[0]
    assert live["in"]["top_asn_packets"] == [{"name": name, "estimate": 18}] == live["out"]["top_asn_packets"]
    assert sum(it["estimate"] for it in live["unknown"]["top_asn_packets"]) == 36
    assert {it["name"] for it in live["unknown"]["top_asn_packets"]} == {name, out}
    assert [it["estimate"] for it in live["in"]["top_geo_loc_packets"]] == [18]


def test_filtered_packets_across_periods_and_slot_reuse(readers):
    """a v2 filter on over 18 periods of 16 slots and in the merged bucket: period p holds p + 1
    passing packets (in) and p + 1 filtered ones (unknown direction)"""
    h = handlers(64, num_periods=2, net2_config={"geoloc_notfound": True})
    try:
        for p in range(18):
            frs = [frame("8.8.8.8", "192.168.0.7"), frame("8.8.8.8", G.OUTSIDE[4])]
            h.process_host(b"".join(record(T0 + 61 * p, k, frs[k % 2]) for k in range(2 * (p + 1))))
        live, prev, merged = (h.bucket_json(h.merge("net", None, p, merged=m))["net"]
                              for p, m in ((0, False), (1, False), (2, True)))
    finally:
        h.close()
    assert (live["filtered_packets"], live["observed_packets"], live["in"]["total_packets"]) == (18, 36, 18)
    assert (prev["filtered_packets"], prev["observed_packets"]) == (17, 34)
    assert (merged["filtered_packets"], merged["observed_packets"], merged["in"]["total_packets"]) == (35, 70, 35)
    assert live["in"]["top_geo_loc_packets"] == [{"name": "Unknown", "estimate": 18}]
    assert merged["in"]["top_geo_loc_packets"] == [{"name": "Unknown", "estimate": 35}] and "unknown" not in merged


def test_external_buckets_sum(readers, model):
    recs = b"".join(record(s, u, f) for s, u, f, _ in G.v1_view(model["pk"]))
    hs = [handlers(len(model["pk"]), num_periods=1) for _ in range(2)]
    try:
        for h in hs:
            h.process_host(recs)
        bucket = hs[0].merge("net", None, 0)
        bucket = hs[1].merge("net", bucket, 0)
        j = hs[0].bucket_json(bucket)["net"]
        prom = hs[0].bucket_prometheus(bucket)
    finally:
        for h in hs:
            h.close()
    assert geo_of(j) == G.expected2(model["pk"] + model["pk"], readers)
    assert 'net_top_asn_packets{asn="1221/Telstra Pty Ltd",direction="out"} 48\n' in prom


def test_deep_sampling_with_the_tops_only(tmp_path, model):
    """deep_sample_rate 50: the geo tops follow the deep-gated IP keys of the same direction"""
    gpu = run(tmp_path, model["pcap"], net2_config={"deep_sample_rate": 50})
    net = gpu["1m"]["net"]
    assert 0 < net["deep_sampled_packets"] < net["observed_packets"] == len(model["pk"])
    for d in G.DIRS:
        ips = sum(it["estimate"] for it in net[d]["top_ipv4_packets"] + net[d]["top_ipv6_packets"])
        assert 0 < ips < sum(it["estimate"] for it in model["v2"][d]["top_asn_packets"])
        assert ips == sum(it["estimate"] for it in net[d]["top_geo_loc_packets"]) == sum(it["estimate"] for it in net[d]["top_asn_packets"])


# ---------------------------------------------------------------- the handler's own filters
def _bracketed(pk, rem):
    """the capture with one packet of `rem` before and after it (the first and the last packet
    pass a filter that passes `rem`: the period's bounds are then the oracle's)"""
    local = "fd00:aaaa::5" if ":" in rem else "192.168.0.7"
    shifted = [(s + 1, u) + tuple(rest) for s, u, *rest in pk]
    return [(T0, 0, frame(rem, local), rem, [("in", rem)])] + shifted + [(T0 + 3, 0, frame(local, rem), rem, [("out", rem)])]


@pytest.mark.parametrize("prefixes,numbers,anchor,passing", [
    (["EU/"], None, "89.160.20.112", {"89.160.20.112", "2a02:dac0::"}),
    (None, ["1221", "7018"], "1.128.0.0", {"1.128.0.0"}),            # "7018" has no slash: 12.81.92.0 is filtered
    (["EU/"], ["29518", "7018"], "89.160.20.112", {"89.160.20.112"}),  # the two families are and-ed
], ids=["geoloc_prefix", "asn_number", "both"])
def test_filters_on_the_synthetic_capture(oracle, tmp_path, readers, model, prefixes, numbers, anchor, passing):
    pk = _bracketed(model["pk"], anchor)
    keep = [p for p in pk if G.passes(readers, p, prefixes, numbers)]
    assert {p[3] for p in keep} == passing
    cfg = {}
    if prefixes is not None:
        cfg["only_geoloc_prefix"] = prefixes
    if numbers is not None:
        cfg["only_asn_number"] = numbers
    gpu = run(tmp_path, pcap_of(G.v1_view(pk)), net2_config=cfg)
    ref = oracle.run_bytes(pcap_of(G.v1_view(keep)), host_spec=HOST, num_periods=1, window=1, topn_count=50, net2_groups=N2_ALL)
    nf = len(pk) - len(keep)
    ref["1m"]["net"]["observed_packets"] += nf
    ref["1m"]["net"]["deep_sampled_packets"] += nf
    ref["1m"]["net"]["filtered_packets"] = nf
    g, r = G.without_geo(gpu)["1m"]["net"], G.without_geo(ref)["1m"]["net"]
    assert diff(g, r) is None, diff(g, r)
    want = G.expected2(keep, readers)
    for d in ("in", "out"):
        assert {k: gpu["1m"]["net"][d][k] for k in GEO} == want[d]
    assert "unknown" not in gpu["1m"]["net"]
    # v1 has its own filter config (none here): it still sees every packet
    full = oracle.run_bytes(pcap_of(G.v1_view(pk)), host_spec=HOST, num_periods=1, window=1, topn_count=50)
    g, r = G.without_geo(gpu)["1m"]["packets"], G.without_geo(full)["1m"]["packets"]
    assert diff(g, r) is None, diff(g, r)


def test_v1_filters_do_not_filter_v2(tmp_path, model, readers):
    gpu = run(tmp_path, model["pcap"], net_config={"only_geoloc_prefix": ["EU/"]}, dns_config={})
    assert gpu["1m"]["packets"]["filtered"] > 0 and gpu["1m"]["net"]["filtered_packets"] == 0
    assert geo_of(gpu["1m"]["net"]) == model["v2"]


def test_a_family_without_its_database_filters_everything(tmp_path, model):
    p = tmp_path / "in.pcap"
    p.write_bytes(model["pcap"])
    j = pa.pktvisor_reader(str(p), host_spec=HOST, periods=1, topn_count=50, net2_config={"asn_notfound": True},
                           geo_city_db=CITY, v2_geo=True)["1m"]
    n = len(model["pk"])
    assert j["net"]["observed_packets"] == j["net"]["filtered_packets"] == j["net"]["deep_sampled_packets"] == n
    assert not any(d in j["net"] for d in G.DIRS)
    assert j["packets"]["filtered"] == 0 and j["packets"]["total"] == n


# ---------------------------------------------------------------- the other outputs
def test_prometheus_and_opentelemetry(model):
    h = handlers(len(model["pk"]), num_periods=1)
    try:
        h.process_host(b"".join(record(s, u, f) for s, u, f, _ in G.v1_view(model["pk"])))
        prom = h.window_prometheus(0, handlers="net")
        otlp = h.window_opentelemetry(0, handlers="net")
    finally:
        h.close()
    assert "# HELP net_top_geo_loc_packets Top GeoIP locations\n# TYPE net_top_geo_loc_packets gauge\n" in prom
    assert "# HELP net_top_asn_packets Top ASNs by IP\n# TYPE net_top_asn_packets gauge\n" in prom
    for d in G.DIRS:
        assert f'net_top_geo_loc_packets{{direction="{d}",geo_loc="EU/Sweden/E/Linköping",lat="58.416700",lon="15.616700"}} 3\n' in prom
        assert f'net_top_geo_loc_packets{{direction="{d}",geo_loc="EU/Russia",lat="60.000000",lon="100.000000"}} 192\n' in prom
        assert f'net_top_asn_packets{{asn="7018",direction="{d}"}} 48\n' in prom
        assert f'net_top_asn_packets{{asn="",direction="{d}"}} 12\n' in prom
    assert 'net_top_asn_packets{asn="Unknown",direction="unknown"} 2579\n' in prom
    for text in (b"net_top_geo_loc_packets", b"net_top_asn_packets", b"geo_loc", b"direction", "EU/Sweden/E/Linköping".encode(),
                 b"58.416700", b"6730/Sunrise Communications AG"):
        assert text in otlp


# ---------------------------------------------------------------- refusals
def test_refusals():
    def refused(match, **kw):
        with pytest.raises(pa.PvError, match=match) as e:
            pa.PvHandlers(host_spec=HOST, num_periods=1, geo_city_db=CITY, geo_asn_db=ISP, **kw)
        assert "(-4)" in str(e.value)
    # without the switch Net v2 with a database is refused, as it always was
    refused("Net v2", net2_config={})
    # with it: sampling with a v2 geo filter
    refused("Net v2 geo filters", v2_geo=True, net2_config={"geoloc_notfound": True, "deep_sample_rate": 50})
    h = handlers(64, num_periods=1)
    try:
        with pytest.raises(pa.PvError, match="dnstap") as e:
            h.process_dnstap(open(os.path.join(GOLD, "fixture.dnstap"), "rb").read())
        assert "(-4)" in str(e.value)
    finally:
        h.close()
    # the filters need the switch
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, net2_config={})
    try:
        with pytest.raises(pa.PvError, match="pv_set_v2_geo"):
            h.set_net_filters(v2=True, geoloc_notfound=True)
    finally:
        h.close()


# ---------------------------------------------------------------- two ranks
def _run_ranks(world, args, timeout=240):
    import subprocess
    import sys
    from tests.dist_launch import ROOT, free_port
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        procs.append(subprocess.Popen([sys.executable, "-m", "tests.geo2_dist_worker", *args], cwd=ROOT, env=env,
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


def test_sharded_run_matches_single_pass(tmp_path, model, readers):
    """Net v2 + DNS v2 on two ranks: the Net capture followed by the DNS pairs, so the cut falls
    near the seam and DNS pairs around it; the reduced window equals the single pass"""
    dpk, dcounted = G.dns2_packets(t0=T0 + 1)
    pcap = model["pcap"] + b"".join(record(s, u, f) for s, u, f, _ in dpk)
    p = tmp_path / "in.pcap"
    p.write_bytes(pcap)
    out = tmp_path / "out.json"
    res = _run_ranks(2, [str(p), str(out), HOST, CITY, ISP])
    assert all(rc == 0 for rc, _ in res), "\n".join(o[-2000:] for _, o in res)
    got = json.load(open(out))["1m"]
    single = pa.pktvisor_reader(str(p), host_spec=HOST, periods=1, topn_count=50, geo_city_db=CITY, geo_asn_db=ISP, v2_geo=True,
                                net2_config={}, dns2_config={"enable": ["top_ecs"]})["1m"]
    want = G.dns2_expected(dcounted, readers)
    for d in G.XDIRS:
        for k in G.GEO2_DNS:
            assert got["dns"][d][k] == want[d][k] == single["dns"][d][k], (d, k)
        assert got["dns"][d]["xacts"] == single["dns"][d]["xacts"]
        for k in GEO:
            assert got["net"][d][k] == single["net"][d][k], (d, k)
        assert got["net"][d]["total_packets"] == single["net"][d]["total_packets"]
    assert got["packets"]["top_ASN"] == single["packets"]["top_ASN"]


def test_sharded_run_refuses_different_databases(tmp_path, model):
    from tests import geo_cases
    p = tmp_path / "in.pcap"
    p.write_bytes(model["pcap"])
    other = tmp_path / "other.mmdb"
    other.write_bytes(R.write_mmdb(geo_cases.V4, 24, 4))
    res = _run_ranks(2, [str(p), str(tmp_path / "out.json"), HOST, CITY, ISP, str(other)])
    assert all(rc != 0 for rc, _ in res)
    assert any("geo databases differ across ranks" in o for _, o in res), "\n".join(o[-1500:] for _, o in res)
    assert not (tmp_path / "out.json").exists()
