"""Flow handler on the GPU: window_json()["flow"] of the device stage (pv_flow_scan /
pv_flow_decode) plus host replay against the Python model (tests/flow_ref.py) over the same records,
and against the reference's known answers on its NetFlow v5 fixture."""
import json
import os

import pytest

import pktvisor_amd as pa
from pktvisor_amd import config as pvcfg
from tests import flow_cases as fc
from tests import flow_ref
from tests.dhcp_ref import records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KAT = json.load(open(os.path.join(GOLDEN, "kat_flow.json")))["nf5.pcap"]
CSV = os.path.join(GOLDEN, "flow_ports.csv")
NF5 = os.path.join(GOLDEN, "nf5.pcap")
T0 = fc.T0
ALL = {"enable": ["all"]}
# classic BPF: keep everything but Ethernet / IPv4 (IHL 5) / UDP with destination port 2056
DROP_2056 = [(0x28, 0, 0, 12), (0x15, 0, 5, 0x800), (0x30, 0, 0, 23), (0x15, 0, 3, 17), (0x28, 0, 0, 36), (0x15, 0, 1, 2056),
             (0x6, 0, 0, 0), (0x6, 0, 0, 262144)]


def rows():
    return pvcfg.iana_port_rows(open(CSV, newline="").read())


def gpu(batches, cfg=None, linktype=1, ts_nano=0, num_periods=5, rate=100, max_events=0, period=0, merged=False, names=False,
        model_batches=None, **kw):
    """the batches through PvHandlers with the flow handler attached: (its window, the model's window, its stats, the model's)"""
    cfg = ALL if cfg is None else cfg
    h = pa.PvHandlers(linktype=linktype, ts_nano=ts_nano, num_periods=num_periods, deep_sample_rate=rate,
                      max_records=max(1, max(len(records(b)) for b in batches)), flow_config=cfg, flow_max_events=max_events,
                      flow_port_csv=CSV if names else None, **kw)
    m = flow_ref.Manager(num_periods, rate, cfg, rows() if names else (), kw.get("topn_count", 10),
                         kw.get("topn_percentile_threshold", 0))
    try:
        for b in batches:
            h.process_host(b)
        for b in (batches if model_batches is None else model_batches):
            m.feed(b, linktype, ts_nano)
        return h.window_json(period, merged)["flow"], m.window(period, merged), h.flow_stats(), m.stats
    finally:
        h.close()


def check(batches, **kw):
    got, want, gs, ws = gpu(batches, **kw)
    assert got == want
    assert gs == ws
    return got, gs


def dgram(version=5, n=2, base=0, sec=T0, frac=0, time=None, **kw):
    return fc.packet(fc.datagram(version, fc.flows_n(n, base), time=(sec, 1000) if time is None else time), sec, frac, **kw)


def test_fixture_known_answers_and_model():
    cfg = {"enable": ["top_tos"]}
    win = pa.pktvisor_reader(NF5, periods=1, flow_config=cfg, flow_port_csv=CSV)["1m"]["flow"]
    assert win["period"]["start_ts"] == KAT["start_ts"]
    assert win["wire_packets"] == {"events": KAT["events"], "deep_samples": KAT["deep_samples"]}
    dev = win["devices"][KAT["device"]]
    assert dev["records_flows"] == KAT["records_flows"]
    ifc = dev["interfaces"][KAT["interface"]]
    assert ifc["cardinality"] == KAT["cardinality"]
    for name, want in KAT["top0"].items():
        for k, v in want.items():
            assert ifc[name][0][k] == v, (name, k)
    lt, ns, recs = pa.read_pcap(NF5)
    m = flow_ref.Manager(1, 100, cfg, rows())
    m.feed(recs, lt, ns)
    last = records(recs)[-1]
    m.set_end(last[1], last[2] * 1000)
    assert win == m.window()


def test_other_handlers_do_not_change():
    both = pa.pktvisor_reader(NF5, periods=1, net_config={}, dns_config={}, flow_config={})["1m"]
    plain = pa.pktvisor_reader(NF5, periods=1, net_config={}, dns_config={})["1m"]
    alone = pa.pktvisor_reader(NF5, periods=1, flow_config={})["1m"]
    assert "flow" not in plain and both["flow"] == alone["flow"]
    assert both["packets"] == plain["packets"] and both["dns"] == plain["dns"]


def test_tiles():
    """a 130-record batch with datagrams at records 0, 63, 64 and 129 and 64-byte UDP filler elsewhere"""
    at = (0, 63, 64, 129)
    batch = b"".join(dgram(5, 1 + at.index(i), i, frac=i) if i in at else fc.filler(T0, i) for i in range(130))
    win, st = check([batch], cfg={"enable": ["all"], "ports": [fc.PORT]})
    assert win["wire_packets"]["events"] == 4 and st == {"datagrams": 4, "invalid": 0, "invalid_v9_v10": 0}
    # on any port the filler is refused, not accepted
    _, st = check([batch])
    assert st == {"datagrams": 4, "invalid": 126, "invalid_v9_v10": 0}


def test_counts_and_versions():
    out = []
    for v in (1, 5, 7):
        mx = fc.MAXFLOWS[v]
        out.append(dgram(v, 1, v))
        out.append(dgram(v, mx, 10 * v))
        out.append(fc.packet(fc.datagram(v, fc.flows_n(2), count=mx + 1), T0))        # count over the maximum
        out.append(fc.packet(fc.datagram(v, fc.flows_n(mx + 1)), T0))                  # and with the records to match
        out.append(fc.packet(fc.datagram(v, [], count=0), T0))
        out.append(fc.packet(fc.datagram(v, fc.flows_n(3), cut=1), T0))                # one short
        out.append(fc.packet(fc.datagram(v, fc.flows_n(3), extra=b"\0"), T0))          # one over
    out.append(fc.packet(fc.datagram(9, fc.flows_n(1)), T0))
    out.append(fc.packet(fc.datagram(10, []), T0))
    out.append(fc.packet(b"\0\5\0", T0))                                               # fewer than a common header
    win, st = check([b"".join(out)], names=True)
    assert st == {"datagrams": 6, "invalid": 18, "invalid_v9_v10": 2}
    assert win["wire_packets"]["events"] == 6 and win["devices"]["10.0.0.2"]["records_flows"] == 2 * 30 + 24 + 3


def test_packet_shapes():
    """a VLAN-tagged exporter, an IPv6 exporter, IPv4 exporters with IHL 6 and 9: the parse_record path,
    the 16-byte device id and the shifted window"""
    batch = (dgram(5, 2, 0, vlan=7, src="10.1.1.1") + dgram(7, 3, 5, v6=True) + dgram(1, 2, 9, ihl=6, src="10.1.1.2") +
             dgram(5, 4, 13, ihl=9, src="10.1.1.3") + dgram(5, 1, 17, ihl=15, src="10.1.1.4") + dgram(5, 1, 21, v6=True, vlan=9))
    win, st = check([batch], cfg={"enable": ["all"], "ports": [fc.PORT]})
    assert st["datagrams"] == 6
    assert set(win["devices"]) == {"10.1.1.1", "2001:db8::2", "10.1.1.2", "10.1.1.3", "10.1.1.4"}
    check([batch])


def test_capture_clipping():
    full = dgram(5, 4, 0)
    n = len(full) - 16
    batch = b"".join(fc.packet(fc.datagram(5, fc.flows_n(4, k)), T0, k, caplen=c) for k, c in enumerate((n, n - 1, n - 48, 60, 45, 43, 42, 30)))
    _, st = check([batch])
    # (caplen 30 leaves no IPv4 header; the others are UDP packets whose clipped payload is refused)
    assert st == {"datagrams": 1, "invalid": 6, "invalid_v9_v10": 0}


def test_port_list():
    batch = dgram(5, 2, 0, dp=2055) + dgram(5, 3, 4, dp=9995) + dgram(5, 1, 8, dp=2056) + dgram(5, 2, 9, sp=2055, dp=4000)
    for ports, n in (([], 4), ([2055], 1), ([9995, 2055], 2), ([1, 2, 3, 4, 5, 6, 7, 2056], 1), ([4000], 1), ([4001], 0)):
        win, st = check([batch], cfg={"enable": ["all"], "ports": ports})
        assert st["datagrams"] == n == win["wire_packets"]["events"]


@pytest.mark.parametrize("max_events", [1, 29, 40, 43, 1000])
def test_decode_rounds(max_events):
    """40: three rounds, and the 30-record datagram that begins in the second one runs past its end"""
    batch = b"".join([dgram(5, 25, 0, frac=1), fc.filler(T0, 2), dgram(5, 17, 30, frac=3), dgram(1, 24, 50, frac=4),
                      dgram(7, 30, 90, frac=5)] + [fc.filler(T0, 6)] * 70 + [dgram(5, 7, 120, frac=7)])
    win, st = check([batch], cfg={"enable": ["all"], "ports": [fc.PORT]}, max_events=max_events)
    assert st["datagrams"] == 5 and win["devices"]["10.0.0.2"]["records_flows"] == 25 + 17 + 30 + 24 + 7


def test_batch_boundary_and_period_shift():
    """two batches whose events straddle a period shift driven by the NetFlow header time"""
    # header times T0 .. T0 + 60; the record that carries T0 + 60 is stamped T0 + 59, so the flow manager
    # shifts on it while the packet handlers' windows (read at the same period) shift one record later
    a = b"".join(dgram(5, 2, i, sec=T0 + 20 * i - (i == 3), time=(T0 + 20 * i, 7)) for i in range(4))
    b = b"".join(dgram(7, 3, 10 + i, sec=T0 + 61 + 30 * i, time=(T0 + 61 + 30 * i, 7)) for i in range(3))
    # (pv_window_json reads one period of every attached handler, and the DNS handler, which shifts on its own
    # events, has none here: the older flow period is read through the merged window)
    live, _ = check([a, b], num_periods=2)
    assert live["wire_packets"]["events"] == 1 and live["period"]["start_ts"] == T0 + 121
    win, _ = check([a, b], num_periods=2, period=2, merged=True)
    assert win["wire_packets"]["events"] == 4  # the merged window of the two newest periods: 3 + 1 events
    one, _ = check([a + b], num_periods=2, period=2, merged=True)
    assert one == win


def test_zero_header_time_takes_the_record_stamp():
    batch = dgram(5, 1, 0, sec=T0, time=(0, 0)) + dgram(5, 1, 1, sec=T0 + 61, time=(0, 0)) + dgram(5, 1, 2, sec=T0 + 62, time=(0, 5))
    win, _ = check([batch], num_periods=3, period=0)
    assert win["period"]["start_ts"] == T0 + 61 and win["wire_packets"]["events"] == 2


def test_deep_sampling():
    pkts = [dgram(5, 3, i, frac=i) for i in range(200)]
    win, _ = check([b"".join(pkts)], rate=50, names=True)
    assert 60 < win["wire_packets"]["deep_samples"] < 140
    check([b"".join(pkts[:77]), b"".join(pkts[77:])], rate=50, max_events=64)


def test_zero_fields():
    flows = fc.zero_flows()
    win, _ = check([fc.packet(fc.datagram(5, flows), T0)], names=True)
    assert win["devices"]["10.0.0.2"]["records_flows"] == 8


def test_groups():
    batch = dgram(5, 20, 0) + dgram(7, 20, 20, src="10.0.0.9")
    for cfg in ({}, {"disable": ["all"]}, {"disable": ["by_bytes"]}, {"disable": ["by_packets", "counters"], "enable": ["conversations"]},
                {"disable": ["all"], "enable": ["top_interfaces", "by_bytes"]}, {"enable": ["top_geo"]}):
        check([batch], cfg=cfg)
    check([batch], topn_count=3, topn_percentile_threshold=50)


def test_bpf_filter_drops_a_datagram():
    batch = dgram(5, 2, 0) + dgram(5, 3, 4, dp=2056) + fc.filler(T0, 5) + dgram(7, 1, 8)
    kept = dgram(5, 2, 0) + fc.filler(T0, 5) + dgram(7, 1, 8)
    win, st = check([batch], bpf=DROP_2056, model_batches=[kept])
    assert st["datagrams"] == 2 and st["invalid"] == 1


def test_reset_starts_over():
    h = pa.PvHandlers(max_records=8, flow_config=ALL)
    try:
        h.process_host(dgram(5, 2, 0) + fc.packet(fc.datagram(9, []), T0))
        assert h.flow_stats() == {"datagrams": 1, "invalid": 1, "invalid_v9_v10": 1}
        h.reset()
        assert h.flow_stats() == {"datagrams": 0, "invalid": 0, "invalid_v9_v10": 0}
        h.process_host(dgram(7, 3, 5))
        m = flow_ref.Manager(5, 100, ALL)
        m.feed(dgram(7, 3, 5))
        assert h.window_json(0)["flow"] == m.window()
    finally:
        h.close()
