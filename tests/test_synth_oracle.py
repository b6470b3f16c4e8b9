"""Oracle sanity on the synthetic configs (CPU)."""
import pytest

from pktvisor_amd import synth


def test_c2_shape(oracle):
    out = oracle.run_bytes(synth.pcap_bytes(2, 20000), host_spec=synth.HOST_SPEC, num_periods=1, window=1)["1m"]
    p = out["packets"]
    assert p["events"] == p["udp"] == p["ipv4"] == 20000
    assert p["in"] + p["out"] + p["unknown_dir"] == 20000
    assert p["payload_size"] == {"p50": 64, "p90": 64, "p95": 64, "p99": 64}
    assert out["dns"]["wire_packets"]["events"] == 0
    assert p["cardinality"]["src_ips_in"] > 1000


def test_c3_shape(oracle):
    out = oracle.run_bytes(synth.pcap_bytes(3, 20000), host_spec=synth.HOST_SPEC, num_periods=1, window=1)["1m"]
    d = out["dns"]["wire_packets"]
    assert d["events"] == d["queries"] == 20000 and d["replies"] == 0
    assert out["dns"]["top_qtype"][0] == {"name": "A", "estimate": 20000}
    sizes = out["packets"]["payload_size"]
    assert 122 <= sizes["p50"] <= 134


@pytest.mark.parametrize("cfg", [1, 4])
def test_paired_configs(oracle, cfg):
    out = oracle.run_bytes(synth.pcap_bytes(cfg, 5000), host_spec=synth.HOST_SPEC, num_periods=1, window=1)["1m"]
    d = out["dns"]
    assert d["wire_packets"]["replies"] > 0
    assert d["xact"]["counts"]["total"] > 0.9 * d["wire_packets"]["replies"]
    assert d["xact"]["out"]["total"] == d["xact"]["counts"]["total"]


def test_edge_mix_runs(oracle):
    out = oracle.run_bytes(synth.pcap_bytes(9, 20000), host_spec="10.0.0.0/8,2000::/3", num_periods=1, window=1)
    assert out["1m"]["packets"]["events"] == 20000


TCP_HOST = "10.0.0.0/8,2001:db8::/32"


def _wire(oracle, pcap):
    return oracle.run_bytes(pcap, host_spec=TCP_HOST, num_periods=1, window=1)["1m"]["dns"]["wire_packets"]


def test_tcp_hole18_is_delivered_by_the_flush_alone(oracle):
    """The inputs of the end-of-capture tests keep discriminating (synth.tcp_hole18_pcap): the
    response behind the 18-byte hole counts once, delivered by closeAllConnections; without the
    held tail nothing is delivered; the noise records are exactly what bpf_progs.SHORT drops, and
    the kept records give the same count."""
    from tests import bpf_progs
    d = _wire(oracle, synth.tcp_hole18_pcap())
    assert (d["tcp"], d["replies"], d["noerror"]) == (1, 1, 1)
    d = _wire(oracle, synth.tcp_hole18_pcap(with_tail=False))
    assert (d["tcp"], d["replies"], d["noerror"]) == (0, 0, 0)
    noisy = synth.tcp_hole18_pcap(noise=40)
    kept = bpf_progs.filter_records(noisy[24:], bpf_progs.SHORT)
    assert kept == synth.tcp_hole18_pcap()[24:]
    assert len(list(synth.records_of(noisy))) == 4 + 40
    d = _wire(oracle, noisy[:24] + kept)
    assert (d["tcp"], d["replies"], d["noerror"]) == (1, 1, 1)


@pytest.mark.parametrize("n_open,late_s,queries,replies", [(24000, 40.0, 8, 60), (24000, 25.0, 12, 60),
                                                           (26000, 40.0, 8, 65), (26000, 25.0, 12, 65)])
def test_tcp_many_open_counts(oracle, n_open, late_s, queries, replies):
    """synth.tcp_many_open_pcap: every 400th connection's response is delivered by a close; the
    four late query completions count at 25 s (nothing is idle) and not at 40 s, where the LRU
    cleanup (100 connections a packet) has closed their connections before the bytes arrive"""
    d = _wire(oracle, synth.tcp_many_open_pcap(n_open, late_s))
    assert (d["queries"], d["replies"], d["tcp"]) == (queries, replies, queries + replies)


def test_split_xact_pairs_once(oracle):
    """synth.split_xact_pcap: one transaction, its query in the first record, its response in the last"""
    pcap = synth.split_xact_pcap()
    recs = list(synth.records_of(pcap))
    assert len(recs) == 202 and synth.is_udp_dns(recs[0][2]) and synth.is_udp_dns(recs[-1][2])
    assert not any(synth.is_udp_dns(r[2]) for r in recs[1:-1])
    out = oracle.run_bytes(pcap, host_spec=TCP_HOST, num_periods=1, window=1)["1m"]["dns"]
    assert out["wire_packets"]["queries"] == out["wire_packets"]["replies"] == 1
    assert out["xact"]["counts"]["total"] == 1


@pytest.mark.parametrize("limit,tcp", [(2, 0), (3, 1), (None, 1)])
def test_tcp_reput_crafted(oracle, limit, tcp):
    """The oracle against the reference's LRU order derived by hand (synth.tcp_reput_pcap): with
    the list capped at 2, closing the evicted A flushes its held fragment, that delivery's put
    evicts B, and B's last segment then belongs to a closed flow (PcapInputStream.cpp:254-263,
    449-465; TcpReassembly::closeConnection). Without the cap, or at 3, B's query counts."""
    out = oracle.run_bytes(synth.tcp_reput_pcap(), num_periods=1, window=1, tcp_packet_reassembly_cache_limit=limit)
    d = out["1m"]["dns"]["wire_packets"]
    assert (d["tcp"], d["queries"]) == (tcp, tcp)
