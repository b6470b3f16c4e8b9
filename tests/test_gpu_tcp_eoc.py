"""The end-of-capture flush (pv_set_end_of_capture, TcpReassembly::closeAllConnections) at its
edges, against the oracle: tens of thousands of connections still open behind a small final batch,
in both LRU modes; a final batch that holds no record (all dropped by the BPF filter, an empty
call, only a partial record behind the last ingest piece); and the flush under deep sampling.
tests/test_synth_oracle.py pins what the inputs must discriminate."""
import struct

import numpy as np
import pytest

import pktvisor_amd as pa
from pktvisor_amd import synth
from tests import bpf_progs
from tests.test_gpu_parity import diff, run_both
from tests.test_gpu_tcp import HOST, _batches

pytestmark = pytest.mark.gpu

# d_fclose holds three words a segment and never less than 65,536 words: a flush past this many
# segments is the first that makes it grow
FCLOSE_FLOOR_SEGS = 65536 // 3


def _window(h, recs, idx=None):
    idx = idx or pa.RecordIndex(recs)
    h.set_end_tstamp(*pa.last_record_ts(recs, idx))
    return {"1m": h.window_json(0)}


def _wire(win):
    return win["1m"]["dns"]["wire_packets"]


# ---------------------------------------------------------------- many open connections
def _many_open(oracle, late_s, exact):
    """synth.tcp_many_open_pcap(26000, late_s) in slices of at most 4,096 records, the last one
    exactly the records stamped >= late_s, armed; returns (gpu window, oracle window)"""
    pcap = synth.tcp_many_open_pcap(26000, late_s)
    rs = synth.records_of(pcap)
    recs = pcap[24:]
    idx = pa.RecordIndex(recs)
    offs = [int(x) for x in idx.offsets] + [len(recs)]
    n_last = sum(1 for sec, usec, _ in rs if sec + usec * 1e-6 >= 1700000000.0 + late_s)
    assert n_last == 20 and idx.n == len(rs)
    first_late = idx.n - n_last
    assert all(sec + usec * 1e-6 < 1700000000.0 + late_s for sec, usec, _ in rs[:first_late])
    bounds = list(range(0, first_late, 4096)) + [first_late, idx.n]
    # the precondition of the d_fclose grow, from the input: every record is a TCP record, none
    # carries FIN or RST, so a connection leaves only by the LRU cleanup, at most 100 a packet and
    # only in the last slice (nothing before it is 30 s idle). No slice before the last reaches the
    # floor; the connections open at the end plus the last slice's segments pass it.
    flows = set()
    for _, _, r in rs:
        f = r[16:]
        assert f[12:14] == b"\x08\x00" and f[23] == 6 and not f[14 + 20 + 13] & 0x05
        ep = sorted([(f[26:30], f[34:36]), (f[30:34], f[36:38])])
        flows.add((ep[0], ep[1]))
    assert len(flows) == 26000 + 8
    assert max(b - a for a, b in zip(bounds[:-2], bounds[1:-1])) <= 4096 < FCLOSE_FLOOR_SEGS
    assert rs[first_late - 1][0] - rs[0][0] < 30
    assert len(flows) - 100 * n_last + n_last > FCLOSE_FLOOR_SEGS
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, max_records=4096, tcp_exact_lru=exact)
    try:
        for a, b in zip(bounds[:-1], bounds[1:]):
            if b == idx.n:
                h.set_end_of_capture()
            h.process_host(recs[offs[a]:offs[b]])
        gpu = _window(h, recs, idx)
    finally:
        h.close()
    return gpu, oracle.run_bytes(pcap, host_spec=HOST, num_periods=1, window=1)


def test_exact_lru_flush_behind_many_open_connections(oracle):
    """the exact LRU mode: the replay's closes of the last slice (the four oldest connections time
    out before their late bytes arrive: 8 queries, not 12) survive the grow of d_fclose that the
    flush segments of some 24,000 open connections force"""
    gpu, ref = _many_open(oracle, 40.0, True)
    assert (_wire(ref)["queries"], _wire(ref)["replies"]) == (8, 65)
    print("queries, replies, tcp:", _wire(gpu)["queries"], _wire(gpu)["replies"], _wire(gpu)["tcp"])
    assert diff(gpu, ref) is None, diff(gpu, ref)


def test_default_mode_flush_behind_many_open_connections(oracle):
    """the default mode at 25 s (nothing is 30 s idle, so the modes' close rules cannot differ):
    the flush takes the segment arrays past max_records and its arena, fragment pool and carry
    hold some 26,000 flush segments"""
    gpu, ref = _many_open(oracle, 25.0, False)
    assert (_wire(ref)["queries"], _wire(ref)["replies"]) == (12, 65)
    print("queries, replies, tcp:", _wire(gpu)["queries"], _wire(gpu)["replies"], _wire(gpu)["tcp"])
    assert diff(gpu, ref) is None, diff(gpu, ref)


# ---------------------------------------------------------------- a final batch without records
def _device_batch(recs):
    import torch
    idx = pa.RecordIndex(recs)
    d_recs = torch.from_numpy(np.frombuffer(recs + bytes(256), dtype=np.uint8).copy()).cuda()
    d_offs = torch.from_numpy(np.ascontiguousarray(idx.offsets[: idx.n])).cuda()
    torch.cuda.synchronize()
    return d_recs, d_offs, idx


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_flush_when_the_filter_empties_the_final_batch(oracle, device):
    """bpf_progs.SHORT drops the whole armed final batch (the 300-byte noise records): the held
    response is still delivered, as the reference's closeAllConnections runs at the end of the file"""
    pcap = synth.tcp_hole18_pcap(noise=40)
    recs = pcap[24:]
    kept = bpf_progs.filter_records(recs, bpf_progs.SHORT)
    head, tail = recs[:len(kept)], recs[len(kept):]
    assert head == kept and bpf_progs.filter_records(tail, bpf_progs.SHORT) == b"" and len(tail) == 40 * (16 + 354)
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, max_records=64, bpf=bpf_progs.SHORT)
    try:
        if device:
            keep = [_device_batch(head), _device_batch(tail)]
            h.process_device(keep[0][0].data_ptr(), keep[0][1].data_ptr(), keep[0][2])
            h.synchronize()
            h.set_end_of_capture()
            h.process_device(keep[1][0].data_ptr(), keep[1][1].data_ptr(), keep[1][2])
            h.synchronize()
        else:
            h.process_host(head)
            h.set_end_of_capture()
            h.process_host(tail)
        gpu = _window(h, kept)
    finally:
        h.close()
    ref = oracle.run_bytes(pcap[:24] + kept, host_spec=HOST, num_periods=1, window=1)
    print("tcp:", _wire(gpu)["tcp"])
    assert _wire(ref)["tcp"] == 1 and _wire(gpu)["tcp"] == 1
    assert diff(gpu, ref) is None, diff(gpu, ref)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_flush_by_an_empty_final_call(oracle, device):
    """the capture in one call, then the armed call with nothing in it: process_host(b"") or
    process_device with a zero-record index"""
    pcap = synth.tcp_hole18_pcap()
    recs = pcap[24:]
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, max_records=64)
    try:
        h.process_host(recs)
        h.set_end_of_capture()
        if device:
            empty = pa.RecordIndex(b"")
            assert empty.n == 0
            h.process_device(0, 0, empty)
            h.synchronize()
        else:
            h.process_host(b"")
        gpu = _window(h, recs)
    finally:
        h.close()
    ref = oracle.run_bytes(pcap, host_spec=HOST, num_periods=1, window=1)
    print("tcp:", _wire(gpu)["tcp"])
    assert _wire(ref)["tcp"] == 1 and _wire(gpu)["tcp"] == 1
    assert diff(gpu, ref) is None, diff(gpu, ref)


def test_flush_by_an_empty_final_call_shifts_the_dns_period(oracle):
    """five periods: a UDP query at 0 s, the hole-18 connection at 70 s. The DNS manager's next
    event after the query is the flushed response, stamped with the connection's end time, so the
    flush of the empty final call is what shifts the DNS period"""
    cli, srv = bytes([10, 0, 0, 1]), bytes([8, 8, 8, 8])
    q = synth._dns_msg(np.random.default_rng(1), 0x0101, False, "early.example.com", 1)
    ev = [(0.0, synth._udp_frame(cli, srv, 40001, 53, q))]
    ev += synth._hole18_events(70.0, cli, 40000, "held.example.com", 0.1)
    pcap = synth._pcap_of(ev)
    recs = pcap[24:]
    h = pa.PvHandlers(host_spec=HOST, num_periods=5, max_records=64)
    try:
        h.process_host(recs)
        h.set_end_of_capture()
        h.process_host(b"")
        h.set_end_tstamp(*pa.last_record_ts(recs, pa.RecordIndex(recs)))
        gpu = {"p0": h.window_json(0), "p1": h.window_json(1), "5m": h.window_json(5, merged=True)}
    finally:
        h.close()
    ref = oracle.run_bytes(pcap, host_spec=HOST, num_periods=5, window=5)
    assert ref["5m"]["dns"]["wire_packets"]["tcp"] == 1
    assert gpu["p0"]["dns"]["wire_packets"]["tcp"] == 1 and gpu["p1"]["dns"]["wire_packets"]["udp"] == 1
    assert diff({"5m": gpu["5m"]}, ref) is None, diff({"5m": gpu["5m"]}, ref)


def test_flush_when_the_last_piece_holds_a_partial_record(oracle, monkeypatch):
    """PV_INGEST_CHUNK_MB=1 and one armed call: the complete records (the hole-18 connection, then
    filler to port 9999, all within one second) total exactly 1 MiB and a 20-byte truncated record
    follows, so the ingest's second piece holds no record and its first was not the last"""
    monkeypatch.setenv("PV_INGEST_CHUNK_MB", "1")
    total = 1 << 20
    ev = synth._hole18_events(0.0, bytes([10, 0, 0, 1]), 40000, "held.example.com", 0.0001)
    size = sum(16 + len(f) for _, f in ev)
    src, dst = bytes([10, 0, 0, 2]), bytes([9, 9, 9, 9])
    k = 0
    while size < total:
        left = total - size
        payload = 1000 if left >= 2 * 1058 else left - 58  # (the last filler lands on the boundary)
        assert 0 <= payload <= 2058
        ev.append((0.001 + 0.0005 * k, synth._udp_frame(src, dst, 50000, 9999, bytes(payload))))
        size += 58 + payload
        k += 1
    pcap = synth._pcap_of(ev)
    recs = pcap[24:]
    rs = synth.records_of(pcap)
    assert len(recs) == total and len({sec for sec, _, _ in rs}) == 1
    partial = struct.pack("<IIII", rs[-1][0], 999999, 1042, 1042) + bytes(4)
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, max_records=1 << 16)
    try:
        h.set_end_of_capture()
        h.process_host(recs + partial)
        gpu = _window(h, recs)
    finally:
        h.close()
    ref = oracle.run_bytes(pcap, host_spec=HOST, num_periods=1, window=1)
    print("tcp:", _wire(gpu)["tcp"])
    assert _wire(ref)["tcp"] == 1 and _wire(gpu)["tcp"] == 1
    assert diff(gpu, ref) is None, diff(gpu, ref)


# ---------------------------------------------------------------- deep sampling
@pytest.mark.parametrize("batched", [False, True], ids=["one_pass", "batches"])
@pytest.mark.parametrize("rate", [1, 50, 99])
def test_flush_under_deep_sampling(oracle, tmp_path, rate, batched):
    """the flushed messages draw in stream order, behind every event of the capture (the TCP stage
    runs ahead of the spans when deep_sample_rate < 100)"""
    pcap = synth.tcp_dns_pcap(0, flows=80, open_tails=16)
    ref = oracle.run_bytes(pcap, host_spec=HOST, num_periods=1, window=1, deep_sample_rate=rate)
    if batched:
        recs = pcap[24:]
        idx = pa.RecordIndex(recs)
        h = pa.PvHandlers(host_spec=HOST, num_periods=1, max_records=512, deep_sample_rate=rate)
        try:
            _batches(h, recs, idx, np.random.default_rng(9))
            gpu = _window(h, recs, idx)
        finally:
            h.close()
    else:
        gpu, _ = run_both(oracle, pcap, HOST, 1, tmp_path, deep_sample_rate=rate)
    assert diff(gpu, ref) is None, diff(gpu, ref)
