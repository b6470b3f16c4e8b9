"""config.net_start with the GeoIP databases marked enabled: the geo filters come back typed
(the pv_net_filters fields) instead of filter_all; without the keyword nothing changes."""
import pytest

from pktvisor_amd import config as pvcfg


def test_typed_filters_when_databases_are_enabled():
    n = pvcfg.net_start({"geoloc_notfound": True, "only_asn_number": ["16509", "22131"]}, geo_enabled=(True, True))
    assert n["filter_all"] is False
    assert n["filters"] == {"geoloc_notfound": True, "asn_notfound": False, "only_geoloc_prefix": None,
                            "only_asn_number": ["16509", "22131"]}
    n = pvcfg.net_start({"only_geoloc_prefix": ["NA/United States"], "asn_notfound": True}, geo_enabled=(True, True))
    assert not n["filter_all"] and n["filters"]["only_geoloc_prefix"] == ["NA/United States"] and n["filters"]["asn_notfound"]
    # a key set to false is no filter
    assert "filters" not in pvcfg.net_start({"geoloc_notfound": False}, geo_enabled=(True, True))
    assert "filters" not in pvcfg.net_start({}, geo_enabled=(True, True))


def test_a_family_without_its_database_filters_everything():
    n = pvcfg.net_start({"asn_notfound": True}, geo_enabled=(True, False))
    assert n["filter_all"] is True and n["filters"]["asn_notfound"]
    n = pvcfg.net_start({"only_geoloc_prefix": ["EU/"]}, geo_enabled=(False, True))
    assert n["filter_all"] is True
    assert pvcfg.net_start({"only_geoloc_prefix": ["EU/"]}, geo_enabled=(True, False))["filter_all"] is False


def test_results_without_the_keyword_are_unchanged():
    for cfg in ({"asn_notfound": True}, {"only_geoloc_prefix": ["NA/US"]}, {"only_asn_number": ["7018"]},
                {"geoloc_notfound": True}):
        n = pvcfg.net_start(dict(cfg))
        assert n["filter_all"] is True and set(n) == {"groups", "filter_all"}
    n = pvcfg.net_start({})
    assert n["filter_all"] is False and set(n) == {"groups", "filter_all"}


@pytest.mark.parametrize("geo", [None, (True, True)])
def test_asn_number_error_text(geo):
    with pytest.raises(pvcfg.ConfigException,
                       match="NetStreamHandler: only_asn_number filter contained an invalid/unsupported value: 16509/Amazon"):
        pvcfg.net_start({"only_asn_number": ["16509/Amazon"]}, geo_enabled=geo)
