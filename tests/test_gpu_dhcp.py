"""DHCP handler on the GPU: window_json()["dhcp"] and the Prometheus text of the device stage
(pv_dhcp_scan / pv_dhcp_decode) plus host replay against the Python model (tests/dhcp_ref.py)
over the same records, and against the reference's known answers on its two fixtures."""
import json
import os

import pytest

import pktvisor_amd as pa
from tests import dhcp_cases as dc
from tests import dhcp_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KAT = json.load(open(os.path.join(GOLDEN, "kat_dhcp.json")))
T0 = dc.T0
# classic BPF: keep everything but Ethernet / IPv4 (IHL 5) / UDP with source or destination port 68
DROP_68 = [(0x28, 0, 0, 12), (0x15, 0, 6, 0x800), (0x30, 0, 0, 23), (0x15, 0, 4, 17), (0x28, 0, 0, 34), (0x15, 3, 0, 68),
           (0x28, 0, 0, 36), (0x15, 1, 0, 68), (0x6, 0, 0, 262144), (0x6, 0, 0, 0)]


def n_records(recs: bytes) -> int:
    return len(dhcp_ref.records(recs))


def gpu(batches, linktype=1, ts_nano=0, num_periods=5, rate=100, ttl_ms=None, max_events=0, period=0, merged=False,
        prom=False, **kw):
    """the batches through PvHandlers with the DHCP handler attached: (its window, the model's window[, Prometheus texts])"""
    cfg = {} if ttl_ms is None else {"xact_ttl_ms": ttl_ms}
    h = pa.PvHandlers(linktype=linktype, ts_nano=ts_nano, num_periods=num_periods, deep_sample_rate=rate,
                      max_records=max(1, max(n_records(b) for b in batches)), dhcp_config=cfg, dhcp_max_events=max_events, **kw)
    m = dhcp_ref.Manager(num_periods, rate, ttl_ms or 5000)
    try:
        for b in batches:
            h.process_host(b)
            m.feed(b, linktype, ts_nano)
        got, want = h.window_json(period, merged)["dhcp"], m.window(period, merged)
        if prom:
            return got, want, h.window_prometheus(period, handlers="dhcp"), dhcp_ref.prometheus(m.window(period))
        return got, want
    finally:
        h.close()


def check(batches, **kw):
    got, want = gpu(batches, **kw)
    assert got == want
    return got


@pytest.mark.parametrize("name", ["dhcp-flow.pcap", "dhcpv6.pcap"])
def test_fixtures_known_answers(name):
    kat = KAT[name]
    path = os.path.join(GOLDEN, name)
    win = pa.pktvisor_reader(path, periods=1, dhcp_config={})["1m"]["dhcp"]
    assert win["period"] == {"start_ts": kat["start"][0], "length": kat["length"]}
    assert win["wire_packets"]["events"] == kat["events"]
    for k, v in kat["counters"].items():
        assert win["wire_packets"][k] == v
    assert [e["name"] for e in win["top_clients"]][:len(kat["top_clients"])] == kat["top_clients"]
    if not kat["top_clients"]:
        assert win["top_clients"] == []
    assert win["top_servers"][0]["name"] == kat["top_servers"][0]
    # and the model, and the other handlers untouched
    lt, ns, recs = pa.read_pcap(path)
    m = dhcp_ref.Manager(1)
    m.feed(recs, lt, ns)
    last = dhcp_ref.records(recs)[-1]
    m.set_end(last[1], last[2] * 1000)
    assert win == m.window()
    both = pa.pktvisor_reader(path, periods=1, net_config={}, dns_config={}, dhcp_config={})["1m"]
    plain = pa.pktvisor_reader(path, periods=1, net_config={}, dns_config={})["1m"]
    assert "dhcp" not in plain and both["dhcp"] == win
    assert both["packets"] == plain["packets"] and both["dns"] == plain["dns"]


def tile_batch(n: int) -> bytes:
    """DHCP packets at records 0, 63, 64 and n - 1, 64-byte non-DHCP UDP packets elsewhere"""
    out = []
    for i in range(n):
        if i in (0, 63, 64, n - 1):
            k = (0, 63, 64, n - 1).index(i)
            out.append(dc.request(50 + k, b"tile%d" % k, T0, i) if k % 2 == 0 else dc.ack(50 + k - 1, "10.9.0.%d" % (k + 1), T0, i))
        else:
            out.append(dc.filler(T0, i))
    return b"".join(out)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_tile_edges(n):
    win = check([tile_batch(n)])
    assert win["wire_packets"]["events"] == len({0, 63, 64, n - 1} & set(range(n)))


@pytest.fixture(scope="module")
def all_dhcp():
    return dc.pair_stream(4097)


def test_every_record_a_dhcp_packet(all_dhcp):
    got, want, ptxt, pref = gpu([all_dhcp], prom=True)
    assert got == want and got["wire_packets"]["events"] == 4097 and got["wire_packets"]["request"] == 2049
    assert len(got["top_clients"]) == 10
    assert ptxt == pref


@pytest.mark.parametrize("max_events", [1, 100, 4096, 4097])
def test_rounds_give_one_json(all_dhcp, max_events):
    assert check([all_dhcp], max_events=max_events)["wire_packets"]["events"] == 4097


def general_path_cases():
    req = dc.bootp(3, 77, opts=[(12, b"general")])
    ackp = dc.bootp(5, 77, "10.7.7.7", op=2, opts=[(54, dc.ip4("10.7.7.1"))])
    off = dc.bootp(2, 78, "10.7.7.8", op=2, opts=[(54, dc.ip4("10.7.7.1"))])
    adv = dc.dhcp6_msg(2, [(1, b"cid"), (2, b"server-duid")])
    c = {}
    c["vlan"] = (1, dc.record(dc.eth(dc.ipv4(dc.udp(req, 68, 67)), vlan=5)) + dc.record(dc.eth(dc.ipv4(dc.udp(off, 67, 68)), src=dc.MAC_S, vlan=5), T0, 1)
                 + dc.record(dc.eth(dc.ipv4(dc.udp(ackp, 67, 68)), src=dc.MAC_S, vlan=5), T0, 2), 3)
    c["ihl6"] = (1, dc.record(dc.eth(dc.ipv4(dc.udp(req, 68, 67), ihl=6))) + dc.record(dc.eth(dc.ipv4(dc.udp(ackp, 67, 68), ihl=6)), T0, 1)
                 + dc.record(dc.eth(dc.ipv4(dc.udp(req, 68, 67), ihl=12)), T0, 2), 3)
    # a non-first fragment whose bytes at the port offsets read 67 / 68, and a first fragment (MF): no UDP layer
    c["fragment"] = (1, dc.record(dc.eth(dc.ipv4(dc.udp(req, 68, 67), frag=0x0010))) + dc.record(dc.eth(dc.ipv4(dc.udp(req, 68, 67), frag=0x2000)), T0, 1)
                     + dc.filler(T0, 2), 0)
    c["v6_hop_by_hop"] = (1, dc.record(dc.eth(dc.ipv6(dc.udp(adv, 547, 546), hop_by_hop=True), 0x86DD, src=dc.MAC_S)), 1)
    c["raw_ip"] = (101, dc.record(dc.ipv4(dc.udp(req, 68, 67))) + dc.record(dc.ipv4(dc.udp(off, 67, 68)), T0, 1)
                   + dc.record(dc.ipv4(dc.udp(ackp, 67, 68)), T0, 2) + dc.record(dc.ipv6(dc.udp(adv, 547, 546)), T0, 3), 4)
    c["v4_ports_over_ipv6"] = (1, dc.record(dc.eth(dc.ipv6(dc.udp(off, 67, 68)), 0x86DD, src=dc.MAC_S)), 1)
    c["v6_ports_over_ipv4"] = (1, dc.record(dc.eth(dc.ipv4(dc.udp(adv, 547, 546)), src=dc.MAC_S)), 1)
    frame = dc.eth(dc.ipv4(dc.udp(dc.bootp(3, 79, opts=[(12, b"cut-short-hostname")]), 68, 67)))
    c["caplen_cut"] = (1, dc.record(frame, caplen=len(frame) - 9) + dc.record(frame, T0, 1, caplen=14 + 20 + 8 + 239)
                       + dc.record(frame, T0, 2, caplen=14 + 20 + 8) + dc.ack(79, sec=T0, frac=3), 4)
    c["hostname_255"] = (1, dc.request(80, bytes(range(1, 256))) + dc.ack(80, sec=T0, frac=1), 2)
    return c


GENERAL = general_path_cases()


@pytest.mark.parametrize("name", sorted(GENERAL))
def test_general_path(name):
    linktype, recs, events = GENERAL[name]
    win = check([recs], linktype=linktype)
    assert win["wire_packets"]["events"] == events
    if name == "raw_ip":
        assert win["top_servers"] == [] and len(win["top_clients"]) == 1 and win["wire_packets"]["advertise"] == 1
    if name == "v6_ports_over_ipv4":
        assert win["top_servers"] == [] and win["wire_packets"]["advertise"] == 1 and win["wire_packets"]["total"] == 0
    if name == "v4_ports_over_ipv6":
        assert win["wire_packets"]["offer"] == 1 and len(win["top_servers"]) == 1
    if name in ("vlan", "ihl6"):
        assert len(win["top_clients"]) == 1
    if name == "v6_hop_by_hop":
        assert win["top_servers"][0]["name"] == "b8:27:eb:0c:b3:e2/fe80::a00:27ff:fed4:10bb"
    if name == "hostname_255":
        assert len(win["top_clients"][0]["name"]) == 17 + 1 + 255 + 1 + len("192.168.2.205")


def test_request_and_ack_in_different_batches():
    win = check([dc.request(1, b"across") + dc.filler(T0, 1), dc.filler(T0 + 1) + dc.ack(1, sec=T0 + 1, frac=5)])
    assert [e["name"] for e in win["top_clients"]] == ["78:4f:43:78:19:bc/across/192.168.2.205"]


def test_one_batch_seven_batches_and_reset():
    recs = dc.pair_stream(700, step_us=300000)  # 210 s: three period shifts
    rs = dhcp_ref.records(recs)
    cuts = [rs[i * len(rs) // 7][0] for i in range(7)] + [len(recs)]
    parts = [recs[cuts[i]:cuts[i + 1]] for i in range(7)]
    one = check([recs], num_periods=3, rate=50)
    assert check(parts, num_periods=3, rate=50) == one
    assert check(parts, num_periods=3, rate=50, period=3, merged=True) == check([recs], num_periods=3, rate=50, period=3, merged=True)
    h = pa.PvHandlers(num_periods=3, deep_sample_rate=50, max_records=len(rs), dhcp_config={})
    try:
        h.process_host(recs)
        first = h.window_json()["dhcp"]
        h.reset()
        h.process_host(recs)
        assert h.window_json()["dhcp"] == first == one
    finally:
        h.close()


def test_bpf_filter_runs_before_the_handler():
    adv = [(1, b"cid"), (2, b"duid")]
    recs = (dc.pair_stream(300) + dc.offer(9, sec=T0 + 1) + dc.filler(T0 + 1, 1) + dc.dhcp6(1, sec=T0 + 1, frac=2)
            + dc.dhcp6(2, adv, sec=T0 + 1, frac=3) + dc.dhcp4(1, 11, T0 + 1, 4, sp=67, dp=67) + dc.filler(T0 + 1, 5))
    kept = pa.bpf_filter(recs, DROP_68)
    assert 0 < n_records(kept) < n_records(recs)
    h = pa.PvHandlers(max_records=n_records(recs), dhcp_config={}, bpf=DROP_68)
    m = dhcp_ref.Manager()
    try:
        h.process_host(recs)
        m.feed(kept)
        assert h.window_json()["dhcp"] == m.window()
        # what is left: the DHCPv6 packets and the relayed (67 to 67) DISCOVER
        assert m.window()["wire_packets"]["events"] == 3 and m.window()["wire_packets"]["total"] == 1
    finally:
        h.close()


def test_device_resident_batch():
    """pv_process_device directly (no ingest in front): the stage hooks there"""
    import numpy as np
    import torch
    recs = tile_batch(257) + dc.pair_stream(130, sec0=T0 + 1)
    idx = pa.RecordIndex(recs)
    d_recs = torch.from_numpy(np.frombuffer(recs + bytes(256), dtype=np.uint8).copy()).cuda()
    d_offs = torch.from_numpy(np.ascontiguousarray(idx.offsets[: idx.n])).cuda()
    h = pa.PvHandlers(max_records=idx.n, dhcp_config={})
    m = dhcp_ref.Manager()
    try:
        h.process_device(d_recs.data_ptr(), d_offs.data_ptr(), idx)
        h.synchronize()
        m.feed(recs)
        assert h.window_json()["dhcp"] == m.window() and m.window()["wire_packets"]["events"] == 134
    finally:
        h.close()


def test_reader_cli_dhcp_flag():
    import subprocess
    exe = os.path.join(ROOT, "pktvisor_amd", "pvgpu-reader")
    path = os.path.join(GOLDEN, "dhcp-flow.pcap")
    out = json.loads(subprocess.check_output([exe, "--periods", "1", "--dhcp", path], timeout=120))["1m"]
    assert out["dhcp"] == pa.pktvisor_reader(path, periods=1, dhcp_config={})["1m"]["dhcp"]
    assert "dhcp" not in json.loads(subprocess.check_output([exe, "--periods", "1", path], timeout=120))["1m"]


def test_deep_sampling_rate_50():
    win = check([dc.pair_stream(2000)], rate=50, num_periods=1)
    assert 800 < win["wire_packets"]["deep_samples"] < 1200 and win["wire_packets"]["events"] == 2000


def test_ttl_from_the_config():
    recs = dc.request(1, b"ttl", T0, 0) + dc.ack(1, sec=T0, frac=900000)
    assert check([recs], ttl_ms=800)["top_clients"] == []
    assert len(check([recs], ttl_ms=1000)["top_clients"]) == 1


def test_refusals():
    from pktvisor_amd import dist as pvdist
    recs = dc.request(1) + dc.ack(1, sec=T0, frac=1)
    h = pa.PvHandlers(max_records=2, dhcp_config={})
    try:
        h.process_host(recs)
        calls = [lambda: h.process_dnstap(b""), lambda: h.window_opentelemetry(handlers="dhcp"),
                 lambda: h.merge("dhcp", None, 0), lambda: pvdist.process_shard(h, recs, pa.RecordIndex(recs), T0)]
        for call in calls:
            with pytest.raises(pa.PvError) as e:
                call()
            assert "(-4)" in str(e.value) and ("DHCP" in str(e.value) or "Dhcp" in str(e.value)), str(e.value)
        # the handler is not attached by default: no "dhcp" object, and the Prometheus default stays net,dns
        assert "dhcp_" not in h.window_prometheus()
        assert "dhcp_wire_packets_total" in h.window_prometheus(handlers="net,dns,dhcp")
    finally:
        h.close()
    p = pa.PvHandlers(max_records=2)
    try:
        p.process_host(recs)
        assert "dhcp" not in p.window_json()
    finally:
        p.close()
