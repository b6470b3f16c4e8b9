"""pv_topn_combine's compact mode: a workgroup whose ranges hold nothing but the lean Net pass's
dense IPv4 entries keeps (address, direction) -> 16-bit count and 16-bit first record index in a
16384-slot LDS table, up to three ranges a workgroup; every other workgroup runs the generic
table. The mode and the fan are choices of speed only, so every window here equals the oracle's
and the windows of PV_CB_FAN=1, PV_CB_FAN=3 and the host's own pick equal one another. The
source / destination cardinalities replay the CPC sketch in first-occurrence order, so a wrong
first record index shows against the oracle."""
import struct

import numpy as np
import pytest

import pktvisor_amd as pa
from tests.test_gpu_parity import diff

pytestmark = pytest.mark.gpu

HOST = "10.0.0.0/8"
T0 = 1700000000
ME = (10 << 24) | 7
ETH = b"\x00\x11\x22\x33\x44\x55\x66\x77\x88\x99\xaa\xbb"
FANS = [None, "1", "3"]  # the host's pick, one range a workgroup, three


def _hdr(ts_us, fr):
    return struct.pack("<IIII", ts_us // 10**6, ts_us % 10**6, len(fr), len(fr)) + fr


def _udp4(src, dst, sport=4000, dport=5000, payload=bytes(22)):
    udp = struct.pack(">HHHH", sport, dport, 8 + len(payload), 0) + payload
    return struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(udp), 0, 0, 64, 17, 0, src, dst) + udp


def _rec(src, dst, ts_us):
    """Ethernet + IPv4 + UDP, no DNS: 64 bytes"""
    return _hdr(ts_us, ETH + b"\x08\x00" + _udp4(src, dst))


def _rec_vlan(src, dst, ts_us):
    return _hdr(ts_us, ETH + b"\x81\x00\x00\x05\x08\x00" + _udp4(src, dst))


def _rec_v6(k, ts_us):
    udp = struct.pack(">HHHH", 4000, 5000, 8 + 22, 0) + bytes(22)
    src = bytes([0x20, 0x01, 0x0d, 0xb8]) + bytes(10) + struct.pack(">H", k)
    dst = bytes([0xfd]) + bytes(14) + b"\x01"
    return _hdr(ts_us, ETH + b"\x86\xdd" + struct.pack(">IHBB", 6 << 28, len(udp), 17, 64) + src + dst + udp)


def _rec_dns(src, dst, ts_us, qid, name=b"\x03www\x07example\x03com\x00"):
    q = struct.pack(">HHHHHH", qid, 0x0100, 1, 0, 0, 0) + name + struct.pack(">HH", 1, 1)
    return _hdr(ts_us, ETH + b"\x08\x00" + _udp4(src, dst, 40000 + qid % 1000, 53, q))


def _remote(k):
    return (20 << 24) + 1 + np.asarray(k, dtype=np.int64) * 7919 % (1 << 24)


def _plain(pairs, t_us, step_us=10):
    return [_rec(int(s), int(d), t_us + k * step_us) for k, (s, d) in enumerate(pairs)]


def _run(batches, fan=None, compact=None, wgcu=None, periods=1, reset_after=(), **kw):
    """the window after each batch of one context (no reset in between)"""
    mp = pytest.MonkeyPatch()
    try:
        for k, v in (("PV_CB_FAN", fan), ("PV_CB_COMPACT", compact), ("PV_NET_WGCU", wgcu)):
            mp.setenv(k, v) if v is not None else mp.delenv(k, raising=False)
        h = pa.PvHandlers(host_spec=HOST, num_periods=periods, max_records=max(len(b) for b in batches) // 80 + 64, **kw)
        out = []
        try:
            for b in batches:
                h.process_host(b)
                h.set_end_tstamp(*pa.last_record_ts(b, pa.RecordIndex(b, max_records=len(b) // 80 + 64)))
                out.append(h.window_json(0))
        finally:
            h.close()
        return out
    finally:
        mp.undo()


def _ref(oracle, batches, upto, **kw):
    return oracle.run_bytes(pa.pcap_file_bytes(b"".join(batches[:upto])), host_spec=HOST, num_periods=1, window=1, **kw)["1m"]


def _edge_pairs():
    """4800 records (75 ranges of 64, 25 groups of three). x: both directions inside one group; y:
    every record of ranges 3..8 (two whole groups), both directions in the second; p: first seen at
    record 191, the last of a range and of a group, q: at record 192, the first of the next, both
    again later; the rest distinct addresses, every third outbound."""
    r = _remote(np.arange(5000))
    x, y, p, q = (int(a) for a in r[4990:4994])
    pairs = [(int(a), ME) if k % 3 else (ME, int(a)) for k, a in enumerate(r[:4800])]
    pairs[10], pairs[20], pairs[150] = (x, ME), (ME, x), (x, ME)
    for k in range(192, 576):
        pairs[k] = (y, ME) if k < 384 or k % 2 else (ME, y)
    pairs[191], pairs[192] = (p, ME), (q, ME)
    pairs[700], pairs[701], pairs[4799] = (ME, p), (q, ME), (p, ME)
    pairs[600], pairs[4000] = (ME, q), (ME, q)
    return pairs


GROUPS = {"default": {}, "no_cardinality": {"net_groups": pa.PV_NET_COUNTERS | pa.PV_NET_TOP_IPS},
          "top_ips_only": {"net_groups": pa.PV_NET_TOP_IPS}}


@pytest.mark.parametrize("groups", list(GROUPS), ids=list(GROUPS))
def test_small_batch_edges(oracle, groups):
    kw = GROUPS[groups]
    batch = b"".join(_plain(_edge_pairs(), T0 * 10**6))
    ref = _ref(oracle, [batch], 1, **kw)
    for fan in FANS:
        got = _run([batch], fan=fan, **kw)[0]
        assert diff(got, ref) is None, (fan, diff(got, ref))
    got = _run([batch], fan="3", compact="0", **kw)[0]  # the generic table at the same fan
    assert diff(got, ref) is None, ("generic", diff(got, ref))


@pytest.mark.parametrize("other", ["ipv6", "vlan", "dns"])
def test_mixed_modes_in_one_launch(oracle, other):
    """a handful of records the compact table cannot hold (an IPv6 key, a general-path record, a
    DNS message's update-log entries) inside some ranges only: those workgroups run the generic
    table, the others of the same launch the compact one"""
    recs = _plain(_edge_pairs(), T0 * 10**6)
    for n, k in enumerate((5, 70, 200, 1000, 1001, 2500, 4700)):
        t = T0 * 10**6 + k * 10
        recs[k] = (_rec_v6(n, t) if other == "ipv6" else
                   _rec_vlan(int(_remote(6000 + n)), ME, t) if other == "vlan" else _rec_dns(int(_remote(6000 + n)), ME, t, 100 + n))
    batch = b"".join(recs)
    ref = _ref(oracle, [batch], 1)
    for fan in FANS:
        got = _run([batch], fan=fan)[0]
        assert diff(got, ref) is None, (fan, diff(got, ref))


def test_prediction_flips(oracle):
    """49152-record batches (768 ranges, so the host groups three a workgroup once the batch before
    was DNS-free): DNS-free, DNS-free (grouped), with DNS messages (grouped on the stale guess:
    their workgroups generic), DNS-free (ungrouped again), DNS-free (grouped), in one window"""
    n = 768 * 64
    r = _remote(np.arange(40000))
    rng = np.random.default_rng(11)
    batches = []
    for b in range(5):
        a = r[rng.zipf(1.3, n) % len(r)]
        recs = _plain([(int(s), ME) if k % 5 else (ME, int(s)) for k, s in enumerate(a)], (T0 + 2 * b) * 10**6)
        if b == 2:
            for j, k in enumerate(range(100, n, 4099)):
                recs[k] = _rec_dns(int(r[j]), ME, (T0 + 2 * b) * 10**6 + k * 10, j)
        batches.append(b"".join(recs))
    refs = [_ref(oracle, batches, k + 1) for k in range(5)]
    wins = {fan: _run(batches, fan=fan) for fan in FANS}
    for fan in FANS:
        for k in range(5):
            assert diff(wins[fan][k], refs[k]) is None, (fan, k, diff(wins[fan][k], refs[k]))
    assert wins["1"] == wins["3"] == wins[None]


HOT = (20 << 24) + (200 << 16) + 1  # 20.200.0.1, outside the addresses _distinct_array counts through


def _distinct_array(n, step_ns, distinct=None, hot=0):
    """n 64-byte UDP records (one 80-byte row each) over the addresses 20.0.0.1 + i % distinct
    (every address its own without it), every third record outbound; the first `hot` records all
    carry HOT instead, inbound"""
    tmpl = np.frombuffer(_rec(0, 0, 0), dtype=np.uint8)
    a = np.tile(tmpl, (n, 1))
    i = np.arange(n, dtype=np.int64)
    t = T0 * 10**9 + i * step_ns
    a[:, 0:4] = (t // 10**9).astype("<u4").view(np.uint8).reshape(n, 4)
    a[:, 4:8] = (t % 10**9 // 1000).astype("<u4").view(np.uint8).reshape(n, 4)
    addr = np.where(i < hot, HOT, (20 << 24) + 1 + i % (distinct or n)).astype(">u4").view(np.uint8).reshape(n, 4)
    me = np.frombuffer(struct.pack(">I", ME), dtype=np.uint8)
    out = ((i % 3 == 0) & (i >= hot))[:, None]
    a[:, 16 + 26:16 + 30] = np.where(out, me, addr)
    a[:, 16 + 30:16 + 34] = np.where(out, addr, me)
    return a


def test_spill_of_a_full_compact_table(oracle):
    """one range a CU (PV_NET_WGCU=1: 256 ranges), 2M distinct addresses, three ranges a workgroup:
    a group holds ~23.4K distinct keys in ~23.4K records, more than the 16384 slots (spill) and
    fewer than 65,536 records"""
    batch = _distinct_array(2_000_000, 5000).tobytes()
    got = _run([batch], fan="3", wgcu="1")[0]
    ref = _ref(oracle, [batch], 1)
    assert diff(got, ref) is None, diff(got, ref)


def test_group_past_the_16bit_bounds(oracle):
    """6M records, one range a CU, three ranges a workgroup forced: a group is ~70.4K records, past
    the 16-bit index and count, so every workgroup must stay on the generic table. The first
    150,000 records (two whole groups and more) carry one address: a compact table taken anyway
    would wrap its count (70,464 -> 4,928 a group) and its record indices, and top_ipv4 and the
    cardinalities' first-occurrence order would differ from the oracle's. The other addresses are
    2M, three times over (6M seen once each leave the library's top_ipv4 empty after its purges
    where the oracle keeps ten, with any combine)."""
    batch = _distinct_array(6_000_000, 5000, 2_000_000, hot=150_000).tobytes()
    got = _run([batch], fan="3", wgcu="1")[0]
    ref = _ref(oracle, [batch], 1)
    assert ref["packets"]["top_ipv4"][0] == {"name": "20.200.0.1", "estimate": 150_000}
    assert diff(got, ref) is None, diff(got, ref)


def test_host_keeps_a_group_within_65535_records(capfd, monkeypatch):
    """the host's own pick, read from the PV_TSTAMPS line's combine workgroup count (the line is
    printed by any build; the cycles in it are zero without -DPV_TSTAMPS). Two ranges a CU of 342
    wave tiles (21,888 records) each: the first batch runs one range a workgroup (nothing known
    of the batch before), the second, after a DNS-free batch, two: three would be 65,664 records.
    Without the bound the pick would be three, which leaves fewer workgroups than CUs and so
    falls back to one."""
    import re
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * cus * 342 * 64
    buf = np.concatenate([_distinct_array(n, 2000, 2_000_000, hot=100_000).ravel(), np.zeros(256, np.uint8)])
    idx = pa.RecordIndex(buf[:n * 80], max_records=n)
    assert idx.n == n
    d_recs, d_offs = torch.from_numpy(buf).cuda(), torch.from_numpy(idx.offsets).cuda()
    torch.cuda.synchronize()
    monkeypatch.setenv("PV_NET_WGCU", "2")
    monkeypatch.setenv("PV_TSTAMPS", "1")
    monkeypatch.delenv("PV_CB_FAN", raising=False)
    monkeypatch.delenv("PV_CB_COMPACT", raising=False)
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, max_records=n)
    try:
        capfd.readouterr()
        for _ in range(2):
            h.process_device(d_recs.data_ptr(), d_offs.data_ptr(), idx)
            h.synchronize()
        w = h.window_json(0)["packets"]
    finally:
        h.close()
    wgs = [int(x) for x in re.findall(r"pv_tstamps combine \((\d+) wg\)", capfd.readouterr().err)]
    assert wgs == [2 * cus, cus], wgs
    assert w["events"] == 2 * n
    assert w["top_ipv4"][0] == {"name": "20.200.0.1", "estimate": 200_000}
