"""The short launch chain of plain lean batches. A lean batch that follows one without a UDP DNS
message and without a deferred record launches only the Net pass, the top-N combine and the merge
(no pv_net_slow_list, DNS pass or names kernel); the combine leaves a batch the guess was wrong
about untouched and the host runs the regular chain on it. The chain is a choice of speed only:
after every batch the window equals the oracle's over the same records (the cardinalities replay
first occurrences, so a wrong order shows) and the window of the same context run with
PV_PLAIN_CHAIN=0, and pv_chain_stats shows the chain each batch took."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import pktvisor_amd as pa
from tests.test_gpu_parity import GOLD, diff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = "10.0.0.0/8,fd00::/8"  # (the IPv6 record's destination is a host address: its source is a top_ipv6 entry)
T0 = 1700000000
ME = (10 << 24) | 7
ETH = b"\x00\x11\x22\x33\x44\x55\x66\x77\x88\x99\xaa\xbb"
QNAME = b"\x03www\x07example\x03com\x00"
N = 4800  # records of a batch: 75 ranges of 64


def _hdr(ts_us, fr):
    return struct.pack("<IIII", ts_us // 10**6, ts_us % 10**6, len(fr), len(fr)) + fr


def _ip4(src, dst, proto, l4):
    return struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(l4), 0, 0, 64, proto, 0, src, dst) + l4


def _udp4(src, dst, sport=4000, dport=5000, payload=bytes(22)):
    return _ip4(src, dst, 17, struct.pack(">HHHH", sport, dport, 8 + len(payload), 0) + payload)


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


def _dns_msg(qid, response=False, name=QNAME):
    return struct.pack(">HHHHHH", qid, 0x8180 if response else 0x0100, 1, 0, 0, 0) + name + struct.pack(">HH", 1, 1)


def _rec_dns(client, ts_us, qid, response=False):
    """a UDP query from the remote client to ME:53, or ME's response to it"""
    port = 40000 + qid % 1000
    if response:
        return _hdr(ts_us, ETH + b"\x08\x00" + _udp4(ME, client, 53, port, _dns_msg(qid, True)))
    return _hdr(ts_us, ETH + b"\x08\x00" + _udp4(client, ME, port, 53, _dns_msg(qid)))


def _tcp4(src, dst, sport, dport, seq, ack, flags, payload=b""):
    tcp = struct.pack(">HHIIBBHHH", sport, dport, seq, ack, 5 << 4, flags, 65535, 0, 0) + payload
    return ETH + b"\x08\x00" + _ip4(src, dst, 6, tcp)


def _tcp_exchange(client, t_us, qid=4242, port=51000):
    """a complete DNS-over-TCP exchange, client -> ME:53: handshake, the query and its response
    (each a two-byte length and the message in one segment), both FINs"""
    q, r = _dns_msg(qid), _dns_msg(qid, True)
    q, r = struct.pack(">H", len(q)) + q, struct.pack(">H", len(r)) + r
    c, s = 1000, 9000
    SYN, ACK, PSH, FIN = 0x02, 0x10, 0x08, 0x01
    fr = [_tcp4(client, ME, port, 53, c, 0, SYN), _tcp4(ME, client, 53, port, s, c + 1, SYN | ACK),
          _tcp4(client, ME, port, 53, c + 1, s + 1, ACK),
          _tcp4(client, ME, port, 53, c + 1, s + 1, PSH | ACK, q),
          _tcp4(ME, client, 53, port, s + 1, c + 1 + len(q), PSH | ACK, r),
          _tcp4(client, ME, port, 53, c + 1 + len(q), s + 1 + len(r), FIN | ACK),
          _tcp4(ME, client, 53, port, s + 1 + len(r), c + 2 + len(q), FIN | ACK),
          _tcp4(client, ME, port, 53, c + 2 + len(q), s + 2 + len(r), ACK)]
    return [_hdr(t_us + 3 * k, f) for k, f in enumerate(fr)]


def _remote(k):
    return (20 << 24) + 1 + np.asarray(k, dtype=np.int64) * 7919 % (1 << 24)


def _plain_recs(b, n=N, span=5000):
    """batch b's n plain records, 10 us apart from second T0 + 2 b: remote addresses drawn (seed b)
    from a pool the batches share, with repeats inside and across batches, every third outbound"""
    rng = np.random.default_rng(100 + b)
    a = _remote(rng.integers(0, span, n))
    t = (T0 + 2 * b) * 10**6
    return [_rec(int(s), ME, t + 10 * k) if k % 3 else _rec(ME, int(s), t + 10 * k) for k, s in enumerate(a)]


def _ts(b, k):
    return (T0 + 2 * b) * 10**6 + 10 * k


def _run(batches, plain=None, periods=1, **kw):
    """one context over the batches (no reset in between): the window and pv_chain_stats after
    each batch; plain="0" sets PV_PLAIN_CHAIN=0"""
    mp = pytest.MonkeyPatch()
    try:
        for k in ("PV_CB_FAN", "PV_CB_COMPACT", "PV_NET_WGCU"):
            mp.delenv(k, raising=False)
        mp.setenv("PV_PLAIN_CHAIN", plain) if plain is not None else mp.delenv("PV_PLAIN_CHAIN", raising=False)
        h = pa.PvHandlers(host_spec=HOST, num_periods=periods, max_records=max(len(b) for b in batches) // 70 + 64, **kw)
        wins, stats = [], []
        try:
            for b in batches:
                h.process_host(b)
                h.set_end_tstamp(*pa.last_record_ts(b, pa.RecordIndex(b, max_records=len(b) // 70 + 64)))
                wins.append(h.window_json(0))
                stats.append(h.chain_stats())
        finally:
            h.close()
        return wins, stats
    finally:
        mp.undo()


def _ref(oracle, batches, upto, **kw):
    return oracle.run_bytes(pa.pcap_file_bytes(b"".join(batches[:upto])), host_spec=HOST, num_periods=1, window=1, **kw)["1m"]


def _check(oracle, batches, want_stats, okw=None, **kw):
    """both runs against the oracle and each other after every batch; the chain each batch took"""
    wins, stats = _run(batches, **kw)
    wins0, stats0 = _run(batches, plain="0", **kw)
    for k in range(len(batches)):
        ref = _ref(oracle, batches, k + 1, **(okw or {}))
        assert diff(wins[k], ref) is None, (k, diff(wins[k], ref))
        assert diff(wins0[k], ref) is None, (k, "PV_PLAIN_CHAIN=0", diff(wins0[k], ref))
        assert wins[k] == wins0[k], (k, diff(wins[k], wins0[k]))
    assert stats == want_stats, stats
    assert stats0 == [(0, 0, 0, k + 1) for k in range(len(batches))], stats0
    return wins


def test_right_guess(oracle):
    """four plain batches: the first runs the regular chain (nothing known of the batch before),
    the others the short chain, none falls back"""
    batches = [b"".join(_plain_recs(b)) for b in range(4)]
    wins = _check(oracle, batches, [(0, 0, 0, 1), (1, 0, 0, 1), (2, 0, 0, 1), (3, 0, 0, 1)])
    assert wins[3]["packets"]["events"] == 4 * N


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_small_grids(oracle, n):
    """one tile, a tile edge, a grid below the CU count: a short-chain batch of n records"""
    batches = [b"".join(_plain_recs(0, 200)), b"".join(_plain_recs(1, n))]
    _check(oracle, batches, [(0, 0, 0, 1), (1, 0, 0, 1)])


def _wrong(case):
    """five plain-shaped batches; batch 3 (index 2) holds what the guess did not expect"""
    recs = [_plain_recs(b) for b in range(5)]
    r = recs[2]
    x = int(_remote(7001))
    if case in ("dns_last", "all"):
        r[N - 1] = _rec_dns(int(_remote(7002)), _ts(2, N - 1), 77)  # the last record of the last range
    if case in ("vlan_first", "all"):
        # the deferred record is the first occurrence of x, which plain records repeat both ways
        r[0] = _rec_vlan(x, ME, _ts(2, 0))
        r[5], r[70], r[3000] = _rec(x, ME, _ts(2, 5)), _rec(ME, x, _ts(2, 70)), _rec(x, ME, _ts(2, 3000))
    if case in ("ipv6", "all"):
        r[1234] = _rec_v6(9, _ts(2, 1234))  # a named entry: the names kernel has work
    if case == "all":
        c = int(_remote(7003))
        r[2000], r[2100] = _rec_dns(c, _ts(2, 2000), 501), _rec_dns(c, _ts(2, 2100), 501, response=True)
    return [b"".join(x) for x in recs]


@pytest.mark.parametrize("case", ["dns_last", "vlan_first", "ipv6", "all"])
def test_wrong_guess(oracle, case):
    """batch 3 starts on the short chain and falls back, batch 4 runs the regular chain, batch 5
    is back on the short chain"""
    wins = _check(oracle, _wrong(case), [(0, 0, 0, 1), (1, 0, 0, 1), (2, 1, 0, 1), (2, 1, 0, 2), (3, 1, 0, 2)])
    assert wins[4]["packets"]["events"] == 5 * N
    if case in ("ipv6", "all"):
        assert wins[4]["packets"]["top_ipv6"] == [{"name": "2001:db8::9", "estimate": 1}]
    if case == "all":
        assert wins[4]["dns"]["xact"]["counts"]["total"] == 1


def test_no_entry_at_all(oracle):
    """top_ips disabled: the lean pass without the IP log, the combine lists nothing and the merge
    has no handler to work for; the status still arrives and the next batch works"""
    kw = {"net_groups": pa.PV_NET_COUNTERS}
    batches = [b"".join(_plain_recs(b)) for b in range(3)]
    wins = _check(oracle, batches, [(0, 0, 0, 1), (1, 0, 0, 1), (2, 0, 0, 1)], okw=kw, **kw)
    assert wins[2]["packets"]["events"] == 3 * N and wins[2]["packets"]["udp"] == 3 * N


def test_tcp53_in_a_plain_batch(oracle):
    """a complete DNS-over-TCP exchange among plain UDP records, no UDP DNS: the batch stays on
    the short chain and the TCP stage behind the read-back decodes the messages"""
    recs = [_plain_recs(b) for b in range(3)]
    ex = _tcp_exchange(int(_remote(7010)), _ts(1, 1000))
    # (the exchange's records are 3 us apart; the plain records behind them start past its last)
    recs[1] =recs[1][:1000] + ex + [_rec(int(_remote(k)), ME, _ts(1, 1003 + k)) for k in range(N - 1000)]
    batches = [b"".join(x) for x in recs]
    wins = _check(oracle, batches, [(0, 0, 0, 1), (1, 0, 0, 1), (2, 0, 0, 1)])
    dns = wins[1]["dns"]
    assert dns["wire_packets"]["tcp"] == 2 and dns["wire_packets"]["udp"] == 0
    assert dns["top_qname2"] == [{"name": ".example.com", "estimate": 2}]


def test_flags_pass_through(oracle):
    """a 4096-entry table flooded by distinct IPv4 addresses on the short chain: full regions
    hand updates to the overflow list and the table is purged, so the overflow and purge words
    the host reads behind the merge are non-zero. The same as the regular chain's window, word
    for word; against the oracle the heavy addresses' estimates lie within the frequent-items
    offset bound tests/test_gpu_topn_bound.py uses."""
    heavy = {int(_remote(9000 + j)): 900 - 60 * j for j in range(10)}
    flood = 30000
    seq = [a for a, c in heavy.items() for _ in range(c)]
    rng = np.random.default_rng(5)
    seq += [int(a) for a in (30 << 24) + 1 + np.arange(flood)]
    seq = [seq[i] for i in rng.permutation(len(seq))]
    t = (T0 + 2) * 10**6
    batches = [b"".join(_plain_recs(0, 1000)),
               b"".join(_rec(a, ME, t + 10 * k) if k % 3 else _rec(ME, a, t + 10 * k) for k, a in enumerate(seq))]
    kw = {"table_log2": 12}
    wins, stats = _run(batches, **kw)
    wins0, stats0 = _run(batches, plain="0", **kw)
    assert stats == [(0, 0, 0, 1), (1, 0, 0, 1)] and stats0 == [(0, 0, 0, 1), (0, 0, 0, 2)]
    assert wins == wins0, diff(wins[1], wins0[1])
    ref = _ref(oracle, batches, 2)
    got, want = wins[1]["packets"], ref["packets"]
    for k in ("events", "udp", "ipv4", "in", "out"):
        assert got[k] == want[k], k
    total = 1000 + len(seq)
    rs = 1 << 12
    bound = 4 * total * rs // (1 << 12) // rs + 2
    top = got["top_ipv4"]
    assert [e["name"] for e in top] == [e["name"] for e in want["top_ipv4"]]
    for e, o in zip(top, want["top_ipv4"]):
        assert o["estimate"] <= e["estimate"] <= o["estimate"] + bound, (e, o, bound)


NOT_ELIGIBLE = {"net_v2": {"net2_config": {}},
                "geoip": {"geo_city_db": os.path.join(GOLD, "GeoIP2-City-Test.mmdb"),
                          "geo_asn_db": os.path.join(GOLD, "GeoIP2-ISP-Test.mmdb")}}


@pytest.mark.parametrize("what", list(NOT_ELIGIBLE))
def test_not_eligible(what):
    batches = [b"".join(_plain_recs(b)) for b in range(3)]
    wins, stats = _run(batches, **NOT_ELIGIBLE[what])
    assert stats == [(0, 0, 0, 1), (0, 0, 0, 2), (0, 0, 0, 3)], stats
    assert wins[2]["packets"]["events"] == 3 * N


def test_general_pass_not_eligible():
    """PV_NET_KERNEL is read once per process, so the forced general pass runs in one of its own"""
    env = dict(os.environ, PV_NET_KERNEL="general")
    env.pop("PV_PLAIN_CHAIN", None)
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_plain_chain"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "kernel pv_net_kernel stats (0, 0, 0, 3) events %d" % (3 * N) in out, out[-3000:]


def test_dhcp_attached(oracle):
    """the DHCP handler's stage is a pass of its own: its context takes the short chain"""
    batches = [b"".join(_plain_recs(b)) for b in range(3)]
    wins, stats = _run(batches, dhcp_config={})
    wins0, stats0 = _run(batches, plain="0", dhcp_config={})
    assert stats == [(0, 0, 0, 1), (1, 0, 0, 1), (2, 0, 0, 1)] and stats0[2] == (0, 0, 0, 3)
    assert wins == wins0
    for k in range(3):
        w = dict(wins[k])
        assert w.pop("dhcp")["wire_packets"]["events"] == 0
        ref = _ref(oracle, batches, k + 1)
        assert diff(w, ref) is None, (k, diff(w, ref))


def test_timing_stamps():
    """on the short chain both dispatch stamps sit on the lean pass"""
    batches = [b"".join(_plain_recs(b)) for b in range(4)]
    mp = pytest.MonkeyPatch()
    mp.delenv("PV_PLAIN_CHAIN", raising=False)
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, max_records=N + 64)
    try:
        h.process_host(batches[0])
        h.set_kernel_timing(1)
        h.kernel_timing(reset=True)
        for b in batches[1:]:
            h.process_host(b)
        ms, launches = h.kernel_timing()
        assert h.chain_stats() == (3, 0, 0, 1)
        assert h.chain_stats(reset=True) == (3, 0, 0, 1) and h.chain_stats() == (0, 0, 0, 0)
        assert launches == 3 and ms > 0, (ms, launches)
        assert h.net_kernel_name() == "pv_net_kernel_reg_tc"
    finally:
        h.close()
        mp.undo()


def _worker():
    import torch
    if torch.cuda.device_count() > 0:
        torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    batches = [b"".join(_plain_recs(b)) for b in range(3)]
    h = pa.PvHandlers(host_spec=HOST, num_periods=1, max_records=N + 64)
    try:
        for b in batches:
            h.process_host(b)
        print("kernel", h.net_kernel_name(), "stats", h.chain_stats(), "events", h.window_json(0)["packets"]["events"])
    finally:
        h.close()
    return 0


if __name__ == "__main__":
    sys.exit(_worker())
