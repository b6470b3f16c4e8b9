"""The top-N count words' "seen" flags (PV_CNT_SEEN_*, pv_layout.h): pv_topn_merge's write-back
skips the IPv4 cardinality coupon and atomicMin of an (address, direction) it has submitted in an
earlier batch. The source / destination cardinalities replay the CPC sketch in first-occurrence
order, so a wrongly skipped minimum, a flag that survives a cleared key or a purge, or a flag
bit read as part of a count shows against the oracle."""
import struct

import numpy as np
import pytest

import pktvisor_amd as pa
from tests.test_gpu_parity import diff

pytestmark = pytest.mark.gpu

HOST = "10.0.0.0/8"
T0 = 1700000000
ME = (10 << 24) | 7  # 10.0.0.7, inside every host spec used here


def _rec(src: int, dst: int, ts_us: int) -> bytes:
    """one pcap record: Ethernet + IPv4 + UDP (ports 4000 -> 5000, no DNS) with 22 payload bytes"""
    udp = struct.pack(">HHHH", 4000, 5000, 8 + 22, 0) + bytes(22)
    ip = struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(udp), 0, 0, 64, 17, 0, src, dst)
    fr = b"\x00\x11\x22\x33\x44\x55\x66\x77\x88\x99\xaa\xbb\x08\x00" + ip + udp
    return struct.pack("<IIII", ts_us // 10**6, ts_us % 10**6, len(fr), len(fr)) + fr


def _batch(pairs, t_us: int, step_us: int = 10) -> bytes:
    return b"".join(_rec(s, d, t_us + k * step_us) for k, (s, d) in enumerate(pairs))


def _remote(k):
    """distinct addresses outside every host spec used here (20.x.y.z)"""
    return (20 << 24) + 1 + np.asarray(k, dtype=np.int64) * 7919 % (1 << 24)


def _inbound(addrs):
    return [(int(a), ME) for a in addrs]


def _outbound(addrs):
    return [(ME, int(a)) for a in addrs]


def _feed(h, batches):
    for b in batches:
        h.process_host(b)


def _end(h, batches):
    recs = batches[-1]
    h.set_end_tstamp(*pa.last_record_ts(recs, pa.RecordIndex(recs)))


def _oracle(oracle, batches, host=HOST, periods=1):
    return oracle.run_bytes(pa.pcap_file_bytes(b"".join(batches)), host_spec=host, num_periods=periods, window=periods)


@pytest.mark.parametrize("table_log2,k", [(12, 1500), (13, 300)], ids=["one_region", "two_regions"])
def test_direction_first_seen_in_a_later_batch(oracle, table_log2, k):
    """batch 1 holds every address only as source, batch 2 only as destination, batch 3 both
    (shuffled) and addresses of its own, batch 4 everything again: each direction's minimum is
    submitted once, in the batch that first has it. 1500 addresses fill a third of the one
    4096-entry region (long probe runs), 300 spread thinly over two."""
    rng = np.random.default_rng(table_log2)
    x, y = _remote(np.arange(k)), _remote(np.arange(k, k + k // 5))
    b3 = _inbound(x) + _outbound(x) + _inbound(y[::2]) + _outbound(y[1::2])
    b4 = _outbound(y) + _inbound(y) + _inbound(x[::-1]) + _outbound(x)
    pairs = [_inbound(np.repeat(x, 2)), _outbound(x[::-1]), [b3[i] for i in rng.permutation(len(b3))],
             [b4[i] for i in rng.permutation(len(b4))]]
    batches = [_batch(p, (T0 + j) * 10**6) for j, p in enumerate(pairs)]
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, table_log2=table_log2, max_records=1 << 17)
    try:
        _feed(h, batches)
        _end(h, batches)
        gpu = {"1m": h.window_json(0)}
    finally:
        h.close()
    ref = _oracle(oracle, batches)
    assert ref["1m"]["packets"]["cardinality"] == {"src_ips_in": pytest.approx(k + k // 5, rel=0.1),
                                                   "dst_ips_out": pytest.approx(k + k // 5, rel=0.1)}
    assert diff(gpu, ref) is None, diff(gpu, ref)


def test_flags_behind_cleared_keys(oracle):
    """18 periods over the same addresses: slot (ordinal mod 16) is cleared (keys only) and used
    again with the count words its first occupants left, flags included. Then reset() and the same
    capture again: both windows equal the oracle's."""
    x = _remote(np.arange(400))
    batches = []
    for p in range(18):
        pairs = _inbound(x) + _outbound(x[::3]) if p % 2 else _outbound(x) + _inbound(x[::3])
        batches.append(_batch(pairs, (T0 + 60 * p) * 10**6, step_us=100))
        batches.append(_batch(_inbound(x[::-1]) + _outbound(x), (T0 + 60 * p + 30) * 10**6, step_us=100))
    ref = _oracle(oracle, batches, periods=5)
    h = pa.PvHandlers(host_spec=HOST, num_periods=5, table_log2=12, max_records=1 << 17)
    try:
        for again in (False, True):
            if again:
                h.reset()
            _feed(h, batches)
            _end(h, batches)
            gpu = {"5m": h.window_json(5, merged=True)}
            assert diff(gpu, ref) is None, (again, diff(gpu, ref))
    finally:
        h.close()


def test_purge_and_recreate(oracle):
    """30000 one-packet addresses through a 4096-entry table: pv_topn_purge drops and the flood
    re-creates entries all the way. The cardinalities stay exact; the heavy addresses stay on top
    inside the purge's bound (test_gpu_topn_bound's), and no estimate carries a flag bit."""
    rng = np.random.default_rng(5)
    heavy = {int(a): 3000 - 100 * j for j, a in enumerate(_remote(np.arange(24)))}
    src = np.concatenate([np.repeat(list(heavy), list(heavy.values())), _remote(np.arange(100, 30100))])
    src = src[rng.permutation(len(src))]
    total = len(src)
    pairs = [(int(a), ME) if j % 3 else (ME, int(a)) for j, a in enumerate(src)]
    batches = [_batch(pairs[i:i + 1000], T0 * 10**6 + i * 10) for i in range(0, total, 1000)]
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, table_log2=12, max_records=1 << 17, topn_count=10)
    try:
        _feed(h, batches)
        _end(h, batches)
        w = h.window_json(0)["packets"]
    finally:
        h.close()
    ref = _oracle(oracle, batches)["1m"]["packets"]
    assert w["cardinality"] == ref["cardinality"]
    assert w["total"] == ref["total"] == total

    def name(a):
        return ".".join(str((a >> s) & 0xff) for s in (24, 16, 8, 0))
    top = w["top_ipv4"]
    assert [e["name"] for e in top] == [name(a) for a in sorted(heavy, key=lambda a: -heavy[a])[:10]]
    bound = 4 * total // 4096 + 2  # each purge removes theta x (half the region) of stored weight
    for e, a in zip(top, sorted(heavy, key=lambda a: -heavy[a])):
        assert heavy[a] <= e["estimate"] <= heavy[a] + bound, (e, heavy[a], bound)
        assert e["estimate"] <= total


def test_base_lowered_mid_window():
    """batch A at global base 1000000, then batch B over the same addresses (another order, some
    of its own) at base 0: B's record indices are the smaller ones, so its minima must reach the
    CPC table although A flagged the entries. The result equals a fresh context that saw B at
    base 0 and then A at base 1000000."""
    rng = np.random.default_rng(9)
    x, y = _remote(np.arange(3000)), _remote(np.arange(3000, 3400))
    a = _inbound(x) + _outbound(x[::2])
    bb = _inbound(np.concatenate([x, y])) + _outbound(np.concatenate([y, x]))
    a = _batch([a[i] for i in rng.permutation(len(a))], T0 * 10**6)
    b = _batch([bb[i] for i in rng.permutation(len(bb))], T0 * 10**6)
    out = []
    for order in (((1000000, a), (0, b)), ((0, b), (1000000, a))):
        h = pa.PvHandlers(host_spec=HOST, num_periods=1, table_log2=13, max_records=1 << 17)
        try:
            for base, recs in order:
                h.set_global_base(base)
                h.process_host(recs)
            w = h.window_json(0)["packets"]
            out.append({k: w[k] for k in ("cardinality", "top_ipv4", "total", "ipv4", "udp")})
        finally:
            h.close()
    assert out[0]["cardinality"]["src_ips_in"] > 3000 and out[0]["cardinality"]["dst_ips_out"] > 3000
    assert diff(out[0], out[1]) is None, diff(out[0], out[1])


def test_general_net_path(oracle):
    """three IPv4 host subnets take the Net pass's general path (the 8-byte IP log in front of the
    combine): the same addresses over four batches, both directions, against the oracle"""
    host = "10.0.0.0/8,192.168.0.0/16,172.16.0.0/12"
    rng = np.random.default_rng(3)
    x = _remote(np.arange(900))
    pairs = [_inbound(x), _outbound(x[::-1]) + _inbound(x[:300]), _inbound(x) + _outbound(x), _outbound(x) + _inbound(x)]
    batches = [_batch([p[i] for i in rng.permutation(len(p))], (T0 + j) * 10**6) for j, p in enumerate(pairs)]
    h = pa.PvHandlers(host_spec=host, num_periods=1, table_log2=12, max_records=1 << 17)
    try:
        _feed(h, batches)
        _end(h, batches)
        gpu = {"1m": h.window_json(0)}
    finally:
        h.close()
    ref = _oracle(oracle, batches, host=host)
    assert diff(gpu, ref) is None, diff(gpu, ref)
