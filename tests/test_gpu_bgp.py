"""BGP handler on the GPU: window_json()["bgp"] and the Prometheus text of the device stage
(pv_bgp_scan / pv_bgp_decode) plus host reassembly against the Python model (tests/bgp_ref.py)
over the same records, and against the reference's known answers on its fixture."""
import json
import os

import pytest

import pktvisor_amd as pa
from tests import bgp_cases as bc
from tests import bgp_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KAT = json.load(open(os.path.join(GOLDEN, "kat_bgp.json")))["bgp.pcap"]
T0 = bc.T0
# classic BPF: keep everything but Ethernet / IPv4 (IHL 5) / TCP with source port 443
DROP_443 = [(0x28, 0, 0, 12), (0x15, 0, 5, 0x800), (0x30, 0, 0, 23), (0x15, 0, 3, 6), (0x28, 0, 0, 34), (0x15, 0, 1, 443),
            (0x6, 0, 0, 0), (0x6, 0, 0, 262144)]


def n_records(recs: bytes) -> int:
    return len(bgp_ref.records(recs))


def gpu(batches, linktype=1, ts_nano=0, num_periods=5, rate=100, max_events=0, period=0, merged=False, prom=False, eoc=False,
        **kw):
    """the batches through PvHandlers with the BGP handler attached: (its window, the model's window[, Prometheus texts])"""
    h = pa.PvHandlers(linktype=linktype, ts_nano=ts_nano, num_periods=num_periods, deep_sample_rate=rate,
                      max_records=max(1, max(n_records(b) for b in batches)), bgp_config={}, bgp_max_events=max_events, **kw)
    m = bgp_ref.Manager(num_periods, rate)
    try:
        for i, b in enumerate(batches):
            last = eoc and i == len(batches) - 1
            if last:
                h.set_end_of_capture()
            h.process_host(b)
            m.feed(b, linktype, ts_nano, last)
        got, want = h.window_json(period, merged)["bgp"], m.window(period, merged)
        if prom:
            return got, want, h.window_prometheus(period, handlers="bgp"), bgp_ref.prometheus(m.window(period))
        return got, want
    finally:
        h.close()


def check(batches, **kw):
    got, want = gpu(batches, **kw)
    assert got == want
    return got


# ---------------------------------------------------------------- 1. fixture
def test_fixture_known_answers():
    path = os.path.join(GOLDEN, "bgp.pcap")
    win = pa.pktvisor_reader(path, periods=1, bgp_config={})["1m"]["bgp"]
    assert win["period"] == {"start_ts": KAT["start"][0], "length": KAT["length"]}
    assert win["wire_packets"]["events"] == KAT["events"] == win["wire_packets"]["deep_samples"]
    for k, v in KAT["counters"].items():
        assert win["wire_packets"][k] == v
    # and the model, and the other handlers untouched
    lt, ns, recs = pa.read_pcap(path)
    m = bgp_ref.Manager(1)
    m.feed(recs, lt, ns, eoc=True)
    last = bgp_ref.records(recs)[-1]
    m.set_end(last[1], last[2] * 1000)
    assert win == m.window()
    both = pa.pktvisor_reader(path, periods=1, net_config={}, dns_config={}, bgp_config={})["1m"]
    plain = pa.pktvisor_reader(path, periods=1, net_config={}, dns_config={})["1m"]
    assert "bgp" not in plain and both["bgp"] == win
    assert both["packets"] == plain["packets"] and both["dns"] == plain["dns"]


# ---------------------------------------------------------------- 2. tile edges
def tile_batch(n: int) -> bytes:
    """one session's records at 0, 1 (the SYNs), 63, 64 and n - 1, 64-byte UDP packets elsewhere"""
    a, b = bc.session()
    at = sorted({0, 1, 63, 64, n - 1} & set(range(n)))
    out = []
    for i in range(n):
        if i in at:
            k = at.index(i)
            p = a if k % 2 == 0 else b
            out.append(p.send(b"", T0, i, bc.SYN) if k < 2 else p.send(bc.bgp_msg(1 + k), T0, i))
        else:
            out.append(bc.filler(T0, i))
    return b"".join(out)


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_tile_edges(n):
    win = check([tile_batch(n)])
    assert win["wire_packets"]["events"] == len({0, 1, 63, 64, n - 1} & set(range(n))) - 2


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_every_record_a_segment_and_none(n):
    got, want, ptxt, pref = gpu([bc.keepalive_stream(n)], prom=True)
    assert got == want and got["wire_packets"]["events"] == n - 2
    assert ptxt == pref and "bgp_wire_packets_keepalive" in ptxt
    none = b"".join(bc.foreign(T0, i) if i % 3 else bc.filler(T0, i) for i in range(n))
    assert check([none])["wire_packets"]["events"] == 0


# ---------------------------------------------------------------- 3. tcp_sec_before
def idle_batch(n, seg_at, foreign_at):
    """a connection opened at records 0..2 (T0), idle, its KEEPALIVE at record seg_at (T0 + 30); a
    foreign TCP record stamped T0 + 30 at foreign_at (None: nowhere); UDP elsewhere"""
    a, _b, syn = bc.opened()
    head = syn + a.send(bc.bgp_msg(1), T0, 2)
    out = [bc.filler(T0, i) for i in range(3, n)]
    out[seg_at - 3] = a.send(bc.bgp_msg(4), T0 + 30, seg_at)
    if foreign_at is not None:
        out[foreign_at - 3] = bc.foreign(T0 + 30, foreign_at)
    return head, out


@pytest.mark.parametrize("seg_at,foreign_at,keepalives", [
    (100, 99, 0),    # the lane just before the segment
    (100, 101, 1),   # the lane just after it
    (100, 40, 0),    # the previous tile
    (100, None, 1),
    (100, 3, 0), (100, 15, 0), (100, 16, 0), (100, 31, 0), (100, 32, 0), (100, 47, 0), (100, 48, 0),  # each row of the tile before
    (64, 63, 0),     # lane 0: the previous tile's last lane
    (64, 65, 1),
    (127, 126, 0),   # lane 63
    (127, 64, 0),    # the tile's lane 0
    (127, 128, 1),   # the next tile
])
def test_tcp_sec_before_is_exact(seg_at, foreign_at, keepalives):
    head, out = idle_batch(130, seg_at, foreign_at)
    win = check([head + b"".join(out)])
    assert win["wire_packets"]["keepalive"] == keepalives and win["wire_packets"]["open"] == 1


def test_tcp_second_of_the_previous_batch():
    head, out = idle_batch(130, 100, None)
    assert check([head + bc.foreign(T0 + 30, 5), b"".join(out)])["wire_packets"]["keepalive"] == 0
    assert check([head + bc.foreign(T0 + 29, 5), b"".join(out)])["wire_packets"]["keepalive"] == 1
    assert check([head + bc.filler(T0 + 30, 5), b"".join(out)])["wire_packets"]["keepalive"] == 1


# ---------------------------------------------------------------- 4. rounds
@pytest.fixture(scope="module")
def stream200():
    recs = bc.keepalive_stream(200)
    m = bgp_ref.Manager()
    m.feed(recs)
    return recs, m.window()


@pytest.mark.parametrize("max_events", [1, 2, 64])
def test_rounds_give_one_json(stream200, max_events):
    recs, want = stream200
    h = pa.PvHandlers(max_records=200, bgp_config={}, bgp_max_events=max_events)
    try:
        h.process_host(recs)
        assert h.window_json()["bgp"] == want and want["wire_packets"]["events"] == 198
    finally:
        h.close()


def test_arena_rerun_with_jumbo_segments():
    """eleven 9,000-byte payloads against a 65,536-byte arena: the round of all 14 segments is rerun over 7 ranks"""
    a, _b, syn = bc.opened()
    recs = syn + b"".join(a.send(bc.bgp_msg(2, bytes([i]) * 8981), T0, 2 + i) for i in range(10))
    a.skip(7)
    recs += a.send(bc.bgp_msg(1, bytes(8981)), T0, 20) + a.send(b"", T0, 21, bc.FIN | bc.ACK)  # held, then flushed by the FIN
    win = check([recs], max_events=16)
    assert win["wire_packets"]["update"] == 10 and win["wire_packets"]["events"] == 10  # (byte 18 of the flushed chunk is 0xff)
    assert check([recs], max_events=0) == win


# ---------------------------------------------------------------- 5. general-path shapes
SHAPES = bc.shapes()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_general_path(name):
    linktype, recs, segments = SHAPES[name]
    win = check([recs], linktype=linktype)
    assert sum(win["wire_packets"][k] for k in ("open", "update", "notification", "keepalive", "routerefresh")) == win["wire_packets"]["total"]
    if segments == 0:
        assert win["wire_packets"]["events"] == 0
    if name in ("vlan", "qinq", "v6", "v6_hop_by_hop", "tcp_options", "v4_in_v6_tunnel", "ihl6_ihl10_ihl12"):
        assert win["wire_packets"]["update"] == 1


def test_non_ethernet_linktype_session():
    a = bc.Peer(40001, 179, 10)
    b = bc.Peer(179, 40001, 90, src=bc.B4, dst=bc.A4)

    def raw(p, pay, frac, flags=bc.PSH | bc.ACK):
        r = bc.record(bc.ipv4(bc.tcp(pay, p.sp, p.dp, p.seq, flags), 6, p.src, p.dst), T0, frac)
        p.skip(len(pay) + (1 if flags & bc.SYN else 0))
        return r
    recs = raw(a, b"", 0, bc.SYN) + raw(b, b"", 1, bc.SYN | bc.ACK) + raw(a, bc.bgp_msg(1), 2) + raw(b, bc.bgp_msg(1), 3) + raw(a, bc.bgp_msg(4), 4)
    win = check([recs], linktype=101)
    assert (win["wire_packets"]["open"], win["wire_packets"]["keepalive"]) == (2, 1)


# ---------------------------------------------------------------- 6. state across batches
def test_connection_and_held_fragments_across_every_cut():
    a, b, syn = bc.opened()
    recs = [syn[:len(syn) // 2], syn[len(syn) // 2:], a.send(bc.bgp_msg(1), T0, 2), b.send(bc.bgp_msg(1), T0, 3)]
    a.skip(10)
    recs += [a.send(bytes([2]) + bytes(25), T0, 4), a.send(bc.bgp_msg(4), T0, 5)]  # held behind a 10-byte hole
    recs += [bc.filler(T0, 6), b.send(bc.bgp_msg(4), T0, 7)]                       # the side changes: flushed
    recs += [a.send(bc.bgp_msg(5), T0 + 1, 8), bc.foreign(T0 + 31, 9), a.send(bc.bgp_msg(2), T0 + 31, 10)]
    one = check([b"".join(recs)])
    assert [one["wire_packets"][k] for k in ("open", "update", "notification", "keepalive", "routerefresh")] == [2, 1, 0, 2, 1]
    for cut in range(1, len(recs)):
        assert check([b"".join(recs[:cut]), b"".join(recs[cut:])]) == one, cut


# ---------------------------------------------------------------- 7. other interactions
def test_bpf_filter_runs_before_the_handler():
    a, _b, syn = bc.opened()
    recs = syn + a.send(bc.bgp_msg(1), T0, 2) + bc.foreign(T0 + 31) + bc.filler(T0 + 31, 1) + a.send(bc.bgp_msg(4), T0 + 31, 2)
    kept = pa.bpf_filter(recs, DROP_443)
    assert n_records(kept) == n_records(recs) - 1
    assert check([recs])["wire_packets"]["keepalive"] == 0  # the foreign record times the connection out
    h = pa.PvHandlers(max_records=n_records(recs), bgp_config={}, bpf=DROP_443)
    m = bgp_ref.Manager()
    try:
        h.process_host(recs)
        m.feed(kept)
        assert h.window_json()["bgp"] == m.window() and m.window()["wire_packets"]["keepalive"] == 1
    finally:
        h.close()


def test_deep_sampling_rate_50():
    win = check([bc.keepalive_stream(2002)], rate=50, num_periods=1)
    assert 800 < win["wire_packets"]["deep_samples"] < 1200 and win["wire_packets"]["events"] == 2000


def test_three_periods_batches_and_reset():
    recs = bc.keepalive_stream(700, step_us=300000)  # 210 s: three period shifts
    rs = bgp_ref.records(recs)
    cuts = [rs[i * len(rs) // 7][0] for i in range(7)] + [len(recs)]
    parts = [recs[cuts[i]:cuts[i + 1]] for i in range(7)]
    one = check([recs], num_periods=3, rate=50)
    assert check(parts, num_periods=3, rate=50) == one and one["period"]["start_ts"] == T0 + 180
    assert check(parts, num_periods=3, rate=50, period=3, merged=True) == check([recs], num_periods=3, rate=50, period=3, merged=True)
    h = pa.PvHandlers(num_periods=3, deep_sample_rate=50, max_records=len(rs), bgp_config={})
    try:
        h.process_host(recs)
        first = h.window_json()["bgp"]
        h.reset()
        h.process_host(recs)
        assert h.window_json()["bgp"] == first == one
    finally:
        h.close()


def test_end_of_capture_flush():
    a, _b, syn = bc.opened()
    recs = syn + a.send(bc.bgp_msg(1), T0, 2)
    a.skip(1)
    recs += a.send(bytes([0, 3]) + bytes(20), T0, 3)
    assert check([recs])["wire_packets"]["notification"] == 0
    assert check([recs], eoc=True)["wire_packets"]["notification"] == 1
    assert check([recs[:len(syn)], recs[len(syn):]], eoc=True)["wire_packets"]["notification"] == 1


def test_end_of_capture_flush_empty_final_batch():
    """the flush stream with bpf=DROP_443: the armed final batch is one record that the filter
    drops, so no record of it reaches the handler; the connections close all the same (the
    reference's closeAllConnections runs at the end of the file whatever the filter kept) and the
    held NOTIFICATION is delivered. The model: the kept records, then an empty final feed."""
    a, _b, syn = bc.opened()
    recs = syn + a.send(bc.bgp_msg(1), T0, 2)
    a.skip(1)
    recs += a.send(bytes([0, 3]) + bytes(20), T0, 3)
    tail = bc.foreign(T0, 4)
    assert pa.bpf_filter(recs, DROP_443) == recs and pa.bpf_filter(tail, DROP_443) == b""
    h = pa.PvHandlers(max_records=n_records(recs), bgp_config={}, bpf=DROP_443)
    m = bgp_ref.Manager()
    try:
        h.process_host(recs)
        m.feed(recs)
        assert h.window_json()["bgp"] == m.window() and m.window()["wire_packets"]["notification"] == 0
        h.set_end_of_capture()
        h.process_host(tail)
        m.feed(b"", eoc=True)
        assert h.window_json()["bgp"] == m.window() and m.window()["wire_packets"]["notification"] == 1
    finally:
        h.close()


def test_device_resident_batch():
    """pv_process_device directly (no ingest in front): the stage hooks there"""
    import numpy as np
    import torch
    recs = tile_batch(129) + bc.keepalive_stream(130, sec0=T0 + 1, port=40002)
    idx = pa.RecordIndex(recs)
    d_recs = torch.from_numpy(np.frombuffer(recs + bytes(256), dtype=np.uint8).copy()).cuda()
    d_offs = torch.from_numpy(np.ascontiguousarray(idx.offsets[: idx.n])).cuda()
    h = pa.PvHandlers(max_records=idx.n, bgp_config={})
    m = bgp_ref.Manager()
    try:
        h.set_kernel_timing(1)
        h.process_device(d_recs.data_ptr(), d_offs.data_ptr(), idx)
        h.synchronize()
        m.feed(recs)
        assert h.window_json()["bgp"] == m.window() and m.window()["wire_packets"]["events"] == 3 + 128
        ms, launches = h.bgp_timing()
        assert launches == 1 and ms > 0
    finally:
        h.close()


def test_reader_cli_bgp_flag():
    import subprocess
    exe = os.path.join(ROOT, "pktvisor_amd", "pvgpu-reader")
    path = os.path.join(GOLDEN, "bgp.pcap")
    out = json.loads(subprocess.check_output([exe, "--periods", "1", "--bgp", path], timeout=120))["1m"]
    assert out["bgp"] == pa.pktvisor_reader(path, periods=1, bgp_config={})["1m"]["bgp"]
    assert "bgp" not in json.loads(subprocess.check_output([exe, "--periods", "1", path], timeout=120))["1m"]


def test_refusals():
    from pktvisor_amd import dist as pvdist
    recs = bc.keepalive_stream(4)
    h = pa.PvHandlers(max_records=4, bgp_config={})
    try:
        h.process_host(recs)
        calls = [lambda: h.process_dnstap(b""), lambda: h.window_opentelemetry(handlers="bgp"),
                 lambda: h.merge("bgp", None, 0), lambda: pvdist.process_shard(h, recs, pa.RecordIndex(recs), T0)]
        for call in calls:
            with pytest.raises(pa.PvError) as e:
                call()
            assert "(-4)" in str(e.value) and ("BGP" in str(e.value) or "Bgp" in str(e.value)), str(e.value)
        with pytest.raises(pa.PvError) as e:
            h.process_dnstap(b"")
        assert "BgpStreamHandler: unsupported input event proxy" in str(e.value)
        # attached after the first batch: refused; not attached by default: no "bgp" object
        with pytest.raises(pa.PvError):
            h.set_bgp()
        assert "bgp_" not in h.window_prometheus()
        assert "bgp_wire_packets_total" in h.window_prometheus(handlers="net,dns,bgp")
    finally:
        h.close()
    p = pa.PvHandlers(max_records=4)
    try:
        p.process_host(recs)
        assert "bgp" not in p.window_json()
    finally:
        p.close()
    with pytest.raises(pa.StreamHandlerException):
        pa.PvHandlers(max_records=4, bgp_config={"xact_ttl_ms": 1})
