"""Flow handler on the GPU: what it does not build is refused with PV_EUNSUPPORTED (-4) and a message
that names the flow handler, never approximated."""
import os

import pytest

import pktvisor_amd as pa
from pktvisor_amd import dist as pvdist
from tests import flow_cases as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CITY = os.path.join(ROOT, "tests", "golden", "GeoIP2-City-Test.mmdb")
T0 = fc.T0
RECS = fc.packet(fc.datagram(5, fc.flows_n(2)), T0) + fc.packet(fc.datagram(7, fc.flows_n(3)), T0, 1)


def refused(call, text):
    with pytest.raises(pa.PvError) as e:
        call()
    assert "(-4)" in str(e.value) and text in str(e.value), str(e.value)


@pytest.fixture()
def h():
    h = pa.PvHandlers(max_records=2, flow_config={})
    h.process_host(RECS)
    yield h
    h.close()


def test_prometheus(h):
    refused(lambda: h.window_prometheus(handlers="flow"), "window_prometheus: not built for the flow handler")
    refused(lambda: h.window_prometheus(handlers="net,dns,flow"), "the flow handler")
    assert "flow" not in h.window_prometheus()  # the default stays net,dns


def test_opentelemetry(h):
    refused(lambda: h.window_opentelemetry(handlers="flow"), "window_opentelemetry: not built for the flow handler")


def test_bucket_merge(h):
    refused(lambda: h.merge("flow", None, 0), "bucket merge: external buckets are not built for the flow handler")


def test_dnstap(h):
    refused(lambda: h.process_dnstap(b""), "FlowStreamHandler: unsupported input event proxy dnstap (the flow handler is attached)")


def test_sharded_run(h):
    refused(lambda: pvdist.process_shard(h, RECS, pa.RecordIndex(RECS), T0), "a flow handler is attached")


def test_top_geo_with_a_database():
    refused(lambda: pa.PvHandlers(max_records=2, flow_config={"enable": ["top_geo"]}, geo_city_db=CITY),
            "the flow handler's top_geo group is not built")
    h = pa.PvHandlers(max_records=2, flow_config={"enable": ["top_geo"]})
    try:
        refused(lambda: h.set_geodb(CITY, None), "the flow handler's top_geo group is not built")
        # without a database nothing is counted, and the four lists are written empty, as the reference writes them
        h.process_host(RECS)
        win = h.window_json(0)["flow"]
        assert win["wire_packets"]["events"] == 2
        ifs = win["devices"]["10.0.0.2"]["interfaces"]
        assert ifs
        for ifc in ifs.values():
            assert {k: v for k, v in ifc.items() if "geo" in k or "asn" in k} == {
                "top_geo_loc_bytes": [], "top_asn_bytes": [], "top_geo_loc_packets": [], "top_asn_packets": []}
    finally:
        h.close()
    # and a database next to a flow handler without top_geo is the Net handler's business alone
    h = pa.PvHandlers(max_records=2, flow_config={}, geo_city_db=CITY)
    try:
        h.process_host(RECS)
        win = h.window_json(0)["flow"]
        assert win["wire_packets"]["events"] == 2
        assert not any("geo" in k or "asn" in k for ifc in win["devices"]["10.0.0.2"]["interfaces"].values() for k in ifc)
    finally:
        h.close()


def test_detached_context_has_no_flow_object():
    h = pa.PvHandlers(max_records=2)
    try:
        h.process_host(RECS)
        assert "flow" not in h.window_json(0)
        # attaching after the first batch is refused
        with pytest.raises(pa.PvError, match="pv_set_flow: call before the first batch"):
            h.set_flow()
    finally:
        h.close()
