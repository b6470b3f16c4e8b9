"""The Net v2 geo model's own conditions and the config typing of the v2 geo switch, on the CPU."""
import pytest

from pktvisor_amd import config as pvcfg
from tests import geo2_cases as G


def test_every_direction_counts_remote_i_three_times_two_to_the_i():
    pk = G.packets2()
    assert len(pk) <= 6000
    cnt = G.counted(pk)
    for d in G.DIRS:
        assert [cnt[d][r] for r in G.REMOTES2] == [3 << i for i in range(len(G.REMOTES2))], d
    # in and out count nothing else; unknown also counts the fixed outside address of each family
    assert set(cnt["in"]) == set(cnt["out"]) == set(G.REMOTES2)
    assert set(cnt["unknown"]) - set(G.REMOTES2) == set(G.OUTSIDE.values())
    # the unknown-direction shapes: source == destination, remote -> remote, the remote on either side
    unk = [p for p in pk if p[3] is None]
    assert sum(1 for p in unk if p[4][0][1] == p[4][1][1]) == 1
    assert sum(1 for p in unk if p[4][0][1] != p[4][1][1] and {p[4][0][1], p[4][1][1]} <= set(G.REMOTES2)) == len(G.PAIRS)
    for fam in (4, 6):
        assert any(p[4][0][1] == G.OUTSIDE[fam] for p in unk) and any(p[4][1][1] == G.OUTSIDE[fam] for p in unk)


def test_estimates_are_distinct_in_every_list():
    rd = G.readers()
    want = G.expected2(G.packets2(), rd)  # (asserts the distinctness itself)
    for d in G.DIRS:
        for key in ("top_geo_loc_packets", "top_asn_packets"):
            est = [it["estimate"] for it in want[d][key]]
            assert len(est) >= 4 and est == sorted(set(est), reverse=True)
        assert {"name": "EU/Sweden/E/Linköping", "estimate": 3, "lat": "58.416700", "lon": "15.616700"} in want[d]["top_geo_loc_packets"]
    from tests.test_gpu_geo_counts import expected
    v1 = expected(G.v1_view(G.packets2()), rd)
    assert v1["top_geoLoc"][1]["estimate"] == 2 * want["in"]["top_geo_loc_packets"][1]["estimate"]


def test_filter_premises():
    rd = G.readers()
    pk = G.packets2()
    keep = [p for p in pk if G.passes(rd, p, ["EU/"], None)]
    assert {p[3] for p in keep} == {"89.160.20.112", "2a02:dac0::"}
    keep = [p for p in pk if G.passes(rd, p, None, ["1221", "7018"])]
    assert {p[3] for p in keep} == {"1.128.0.0"}  # "7018" has no slash in the database


def test_net2_start_types_the_filters_with_the_switch():
    assert pvcfg.net2_start({}) == pvcfg.net2_start({}, geo=True)["groups"]
    assert pvcfg.net2_start({}, geo=True)["filters"] is None
    out = pvcfg.net2_start({"geoloc_notfound": True, "only_asn_number": ["16509", "22131"], "disable": ["top_ips"]}, geo=True)
    assert out["filters"] == {"geoloc_notfound": True, "asn_notfound": False, "only_geoloc_prefix": None,
                              "only_asn_number": ["16509", "22131"]}
    assert out["groups"] == pvcfg.net2_start({"disable": ["top_ips"]})
    assert pvcfg.net2_start({"only_geoloc_prefix": []}, geo=True)["filters"]["only_geoloc_prefix"] == []
    with pytest.raises(pvcfg.ConfigException, match="only_asn_number filter contained an invalid/unsupported value: 16509/Amazon"):
        pvcfg.net2_start({"only_asn_number": ["16509/Amazon"]}, geo=True)
    with pytest.raises(pvcfg.ConfigException, match="wrong type for key: geoloc_notfound"):
        pvcfg.net2_start({"geoloc_notfound": 1}, geo=True)


def test_dns2_start_types_the_flags_with_the_switch():
    out = pvcfg.dns2_start({"geoloc_notfound": True}, geo=True)
    assert out["v2_geo"] == {"geoloc_notfound": True, "asn_notfound": False}
    assert pvcfg.dns2_start({}, geo=True)["v2_geo"] == {"geoloc_notfound": False, "asn_notfound": False}
    assert "v2_geo" not in pvcfg.dns2_start({})


@pytest.mark.parametrize("key,val", [("geoloc_notfound", True), ("asn_notfound", True), ("only_geoloc_prefix", ["EU/"]),
                                     ("only_asn_number", ["1221"])])
def test_defaults_still_raise(key, val):
    with pytest.raises(pvcfg.ConfigException, match=f"{key} is not supported by the GPU Net v2 handler"):
        pvcfg.net2_start({key: val})
    if key.endswith("notfound"):
        with pytest.raises(pvcfg.ConfigException, match=f"{key} is not supported by the GPU DNS v2 handler"):
            pvcfg.dns2_start({key: val})


# ---------------------------------------------------------------- the DNS v2 model
def test_dns2_model_counts_and_distinct_estimates():
    rd = G.readers()
    pk, counted = G.dns2_packets()
    assert len(pk) <= 6000
    for d in G.XDIRS:
        per = [sum(1 for dd, s in counted if dd == d and s == sub) for sub in G.SUBNETS2]
        # (the one TCP pair rides on the last subnet, direction out)
        assert per == [3 << i for i in range(len(G.SUBNETS2) - 1)] + [(3 << (len(G.SUBNETS2) - 1)) + (d == "out")], d
    want = G.dns2_expected(counted, rd)  # (asserts the distinctness itself)
    assert all(len(want[d][k]) >= 3 for d in G.XDIRS for k in G.GEO2_DNS)
    # both families of ECS travel, and every third pair over IPv6
    assert {s[0] for _, s in counted} == {1, 2}


@pytest.mark.parametrize("keep,flag", [("city", "geoloc_notfound"), ("asn", "asn_notfound")])
def test_exactly_the_keep_queries_pass_the_filter(keep, flag):
    """the premise of the filter-equivalence test: with the independent reader, exactly the
    queries named keep.example.com pass geoloc_notfound (asn_notfound with its own capture)"""
    rd = G.readers()
    pk, _ = G.dns2_packets(keep=keep, rd=rd)
    seen = {True: 0, False: 0}
    for _, _, fr, isq in pk:
        m = G.D.udp_dns_message(fr)
        if m is None or not isq:
            continue  # (the TCP pair's query is checked below)
        ecs = G.D.ecs_of_message(m)
        passing = ecs is not None and ecs[0] in (1, 2) and G.D.passes(rd, (ecs[0], ecs[1]), **{flag: True})
        named = b"\x04keep\x07example\x03com\x00" in m
        assert passing == named
        seen[named] += 1
    assert seen[True] > 50 and seen[False] > 50
    tcp_named = G.D.lookup(rd, keep, G.SUBNETS2[-1])[0] == "Unknown"
    tcp_q = [fr for _, _, fr, isq in pk if isq and G.D.udp_dns_message(fr) is None]
    assert len(tcp_q) == 1 and (b"\x04keep\x07example\x03com\x00" in tcp_q[0]) == tcp_named
