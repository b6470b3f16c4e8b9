"""The model of the DNS v1 handler's top_geoLoc_ecs / top_asn_ecs (tests/dns_geo_cases.py) and the
config plumbing of the DNS geo switch, without a GPU: the model on the reference's ecs.pcap
(src/handlers/dns/v1/tests/test_dns_layer.cpp:711-854), the synthetic capture's own assertions,
and pktvisor_amd.config.dns_start with and without the switch."""
import os

from pktvisor_amd import config as pvcfg
from tests import dns_geo_cases as C

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CITY = os.path.join(GOLD, "GeoIP2-City-Test.mmdb")
ISP = os.path.join(GOLD, "GeoIP2-ISP-Test.mmdb")
U5 = [{"name": "Unknown", "estimate": 5}]


def test_model_on_the_reference_capture():
    """ecs.pcap: five UDP queries carry the subnet 2001:470:1f0b:1600::, which neither test database holds"""
    rd = C.readers(CITY, ISP)
    subs = []
    for fr in C.pcap_frames(open(os.path.join(GOLD, "ecs.pcap"), "rb").read()):
        m = C.udp_dns_message(fr)
        sub = C.ecs_of_message(m) if m is not None else None
        if sub:
            subs.append(sub)
    assert len(subs) == 5 and {C.subnet_text(s) for s in subs} == {"2001:470:1f0b:1600::"}
    pk = [(0, 0, b"", s) for s in subs]
    want = C.expected(pk, rd)
    assert want["top_geoLoc_ecs"] == U5 and want["top_asn_ecs"] == U5
    assert C.expected_query_ecs(pk) == [{"name": "2001:470:1f0b:1600::", "estimate": 5}]


def test_address_rule():
    assert C.full_address(C.v4("1.128.0.0", 3)) == bytes([1, 128, 0, 0])
    assert C.full_address(C.v4("81.2.69.142", 4, b"\xde\xad")) == bytes([81, 2, 69, 142])
    assert C.subnet_text(C.v6("2001:db8::77")) == "2001:db8::"  # bytes 9..16 are never copied
    assert C.subnet_text(C.v6("2001:1700::", 16, b"\xff" * 8)) == "2001:1700::"
    assert C.subnet_text(C.v6("2001:218::", 4)) == "2001:218::"
    # the builders and the decoder agree
    for sub in C.SUBNETS:
        m = C.udp_dns_message(C.ecs_query(9, sub, six=sub[0] == 2))
        assert C.ecs_of_message(m) == sub
    assert C.ecs_of_message(C.message(1, "a.b", C.opt_rr(C.ecs_option(3, b"\x01\x02")))) is None
    assert C.ecs_of_message(C.message(1, "a.b", C.opt_rr(C.ecs_option(1, b"\x01\x02")), qr=1)) is None
    assert C.ecs_of_message(C.message(1, "a.b", C.opt_rr())) is None
    assert C.ecs_of_message(C.message(1, "a.b")) is None


def test_synthetic_capture():
    rd = C.readers(CITY, ISP)
    pk = C.packets()
    want = C.expected(pk, rd)  # (asserts that the per-key counts are distinct)
    n = len(C.counted(pk))
    assert n == 3 * (2 ** len(C.SUBNETS) - 1) + 1 and len(pk) == n + 5 + 1
    for k in ("top_geoLoc_ecs", "top_asn_ecs"):
        assert sum(it["estimate"] for it in want[k]) == n
    assert {"name": "EU/Sweden/E/Linköping", "estimate": 3, "lat": "58.416700", "lon": "15.616700"} in want["top_geoLoc_ecs"]
    names = [it["name"] for it in want["top_asn_ecs"]]
    assert "" in names and "Unknown" in names and "7018" in names and "1221/Telstra Pty Ltd" in names
    assert sum(it["estimate"] for it in C.expected_query_ecs(pk)) == n
    # the wave aggregation's fall-through path (more than four (slot, id) groups among 64 lanes) is
    # reached: a run of 64 consecutive ECS queries holds at least six distinct dictionary entries
    subs = C.counted(pk)
    for kind in ("city", "asn"):
        assert max(len({C.lookup(rd, kind, s) for s in subs[a:a + 64]}) for a in range(0, 256, 64)) >= 6, kind
    # the filters' passing sets are neither empty nor everything
    for kw in ({"geoloc_notfound": True}, {"asn_notfound": True}, {"geoloc_notfound": True, "asn_notfound": True}):
        keep = [p for p in pk if C.passes(rd, p[3], **kw)]
        assert 0 < len(keep) < n
        assert all(C.lookup(rd, "city" if "geoloc_notfound" in kw else "asn", p[3])[0] == "Unknown" for p in keep)
    assert not [p for p in pk if C.passes(rd, p[3], geoloc_notfound=True, city=False)]


def test_config_dns_start_types_the_geo_filters():
    cfg = {"enable": ["top_ecs"], "geoloc_notfound": True, "only_queries": True}
    d = pvcfg.dns_start(dict(cfg), dns_geo=True)
    assert d["dns_geo"] == {"enable": 1, "geoloc_notfound": 1, "asn_notfound": 0}
    assert d["filters"]["filter_all"] == 0 and d["filters"]["only_queries"] == 1
    d = pvcfg.dns_start({"asn_notfound": True, "geoloc_notfound": False}, dns_geo=True)
    assert d["dns_geo"] == {"enable": 1, "geoloc_notfound": 0, "asn_notfound": 1}
    assert pvcfg.dns_start({}, dns_geo=True)["dns_geo"] == {"enable": 1, "geoloc_notfound": 0, "asn_notfound": 0}


def test_config_dns_start_without_the_switch_is_unchanged():
    cfg = {"enable": ["top_ecs"], "geoloc_notfound": True, "only_queries": True}
    d = pvcfg.dns_start(dict(cfg))
    assert set(d) == {"groups", "filters", "xact_ttl_ms", "dnstap_mask"}
    assert d["filters"]["filter_all"] == 1 and d["filters"]["only_queries"] == 1
    assert pvcfg.dns_start(dict(cfg), dns_geo=False) == d
    assert pvcfg.dns_start({})["filters"]["filter_all"] == 0
