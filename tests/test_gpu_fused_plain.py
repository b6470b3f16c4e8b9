"""pv_net_combine_plain: on the plain short chain the lean Net pass and the top-N combine of a
batch run as one launch when the combine's groups are the Net workgroups' own ranges (three ranges
a workgroup, one workgroup a CU, so 3 C ranges on a device of C CUs), except on a dispatch-stamped
batch. A choice of speed only: after every batch the window equals the oracle's over the same
records (the cardinalities replay first occurrences, so a wrong record index shows) and the window
of the same context run with PV_FUSE_PLAIN=0, and pv_fuse_stats shows the launch each batch took.

An exception-list entry cannot reach a fused launch: only a general-path record (an IPv6 key)
makes one, and the lean pass defers every such record, which sends the batch to the regular
chain. The generic table inside the fused kernel is covered through PV_CB_COMPACT=0 with
PV_CB_FAN=3 (test_generic_table_in_a_fused_launch)."""
import os
import struct

import numpy as np
import pytest

import pktvisor_amd as pa
from tests.test_gpu_parity import GOLD, diff

pytestmark = pytest.mark.gpu

HOST = "10.0.0.0/8,fd00::/8"  # (the IPv6 record's destination is a host address)
T0 = 1700000000
ME = (10 << 24) | 7
ETH = b"\x00\x11\x22\x33\x44\x55\x66\x77\x88\x99\xaa\xbb"
GROUPS = {"default": {}, "no_cardinality": {"net_groups": pa.PV_NET_COUNTERS | pa.PV_NET_TOP_IPS},
          "top_ips_only": {"net_groups": pa.PV_NET_TOP_IPS}}


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


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


def _rows(addr, out, t0_us, step_us=10):
    """one 80-byte row (64-byte UDP record) per remote address: inbound (addr -> ME), or outbound
    where `out` is set; record k at t0_us + k * step_us"""
    n = len(addr)
    a = np.tile(np.frombuffer(_rec(0, 0, 0), dtype=np.uint8), (n, 1))
    t = t0_us + np.arange(n, dtype=np.int64) * step_us
    a[:, 0:4] = (t // 10**6).astype("<u4").view(np.uint8).reshape(n, 4)
    a[:, 4:8] = (t % 10**6).astype("<u4").view(np.uint8).reshape(n, 4)
    ad = np.asarray(addr, dtype=np.int64).astype(">u4").view(np.uint8).reshape(n, 4)
    me = np.frombuffer(struct.pack(">I", ME), dtype=np.uint8)
    o = np.asarray(out, dtype=bool)[:, None]
    a[:, 16 + 26:16 + 30] = np.where(o, me, ad)
    a[:, 16 + 30:16 + 34] = np.where(o, ad, me)
    return a


def _t(b, k=0):
    return (T0 + 2 * b) * 10**6 + 10 * k


def _plain_rows(b, n, span=5000):
    """batch b's n plain records from second T0 + 2 b: remote addresses drawn (seed b) from a pool
    the batches share, with repeats inside and across batches, every third outbound"""
    rng = np.random.default_rng(100 + b)
    return _rows(_remote(rng.integers(0, span, n)), np.arange(n) % 3 == 0, _t(b))


def _with(rows, subs):
    """the batch's bytes with record k replaced by subs[k] (any length)"""
    out, at = [], 0
    for k in sorted(subs):
        out += [rows[at:k].tobytes(), subs[k]]
        at = k + 1
    return b"".join(out + [rows[at:].tobytes()])


def _run(batches, fuse=None, env=(), timing=0, **kw):
    """one context over the batches (no reset in between): the window and pv_fuse_stats after each
    batch; fuse="0" sets PV_FUSE_PLAIN=0; timing: pv_set_kernel_timing's period, set first"""
    mp = pytest.MonkeyPatch()
    try:
        for k in ("PV_CB_FAN", "PV_CB_COMPACT", "PV_NET_WGCU", "PV_PLAIN_CHAIN", "PV_FUSE_PLAIN"):
            mp.delenv(k, raising=False)
        for k, v in dict(env).items():
            mp.setenv(k, v)
        if fuse is not None:
            mp.setenv("PV_FUSE_PLAIN", fuse)
        h = pa.PvHandlers(host_spec=HOST, num_periods=1, max_records=max(len(b) for b in batches) // 80 + 64, **kw)
        wins, stats = [], []
        try:
            if timing:
                h.set_kernel_timing(timing)
            for b in batches:
                h.process_host(b)
                h.set_end_tstamp(*pa.last_record_ts(b, pa.RecordIndex(b, max_records=len(b) // 80 + 64)))
                wins.append(h.window_json(0))
                stats.append(h.fuse_stats())
            ktime = h.kernel_timing()
        finally:
            h.close()
        return wins, stats, ktime
    finally:
        mp.undo()


def _ref(oracle, batches, upto, **kw):
    return oracle.run_bytes(pa.pcap_file_bytes(b"".join(batches[:upto])), host_spec=HOST, num_periods=1, window=1, **kw)["1m"]


def _check(oracle, batches, want_stats, okw=None, strip=None, **kw):
    """both runs against the oracle and each other after every batch; the launch each batch took"""
    wins, stats, _ = _run(batches, **kw)
    wins0, stats0, _ = _run(batches, fuse="0", **kw)
    f = strip or (lambda w: w)
    for k in range(len(batches)):
        ref = _ref(oracle, batches, k + 1, **(okw or {}))
        assert diff(f(wins[k]), f(ref)) is None, (k, diff(f(wins[k]), f(ref)))
        assert diff(f(wins0[k]), f(ref)) is None, (k, "PV_FUSE_PLAIN=0", diff(f(wins0[k]), f(ref)))
        assert wins[k] == wins0[k], (k, diff(wins[k], wins0[k]))
    assert stats == want_stats, stats
    assert stats0 == [(0, 0)] * len(batches), stats0
    return wins


def _fusable(n, cus):
    """the host's pick for a plain batch of n records after a plain one: three ranges a CU, three
    ranges a combine workgroup while a group stays within 65,535 records and every CU gets one,
    and as many combine workgroups as Net workgroups (one a CU)"""
    tiles = (n + 63) // 64
    grid = min(tiles, 3 * cus)
    wt = (tiles + grid - 1) // grid
    grid = (tiles + wt - 1) // wt
    f = min(3, 65535 // (wt * 64))
    return f > 1 and (grid + f - 1) // f >= cus and (grid + f - 1) // f == min(grid, cus)


@pytest.mark.parametrize("groups", list(GROUPS), ids=list(GROUPS))
@pytest.mark.parametrize("shape", ["one_tile", "ragged", "plus_one"])
def test_smallest_shapes(oracle, groups, shape):
    """3 C ranges of one tile; of two tiles with a ragged last tile and a short last group; one
    record more than 3 C tiles (two tiles a range, 1.5 C ranges: too few groups, so unfused). The
    first batch has no guess yet and runs unfused."""
    c = _cus()
    n = {"one_tile": 3 * c * 64, "ragged": 3 * c * 64 * 2 - 37, "plus_one": 3 * c * 64 + 1}[shape]
    assert _fusable(n, c) == (shape != "plus_one")
    batches = [_plain_rows(b, n).tobytes() for b in range(2)]
    kw = GROUPS[groups]
    _check(oracle, batches, [(0, 0), (1, 0) if shape != "plus_one" else (0, 0)], okw=kw, **kw)


def test_first_occurrence_across_edges(oracle):
    """3 C ranges of 64 records, groups of 192. x: both directions inside one group; y: every record
    of ranges 4 and 5 (two whole ranges), both directions in the second; p: first seen at record
    191, the last of a range and of a group, q: at record 192, the first of the next, both again
    later in other groups; the rest distinct addresses, every third outbound"""
    n = 3 * _cus() * 64
    r = _remote(np.arange(n + 10))
    x, y, p, q = (int(a) for a in r[n + 1:n + 5])
    addr, out = r[:n].copy(), np.arange(n) % 3 == 0
    for k, a, o in ((10, x, 0), (20, x, 1), (150, x, 0), (191, p, 0), (192, q, 0), (700, p, 1), (701, q, 0), (n - 1, p, 0),
                    (600, q, 1), (4000, q, 1)):
        addr[k], out[k] = a, bool(o)
    addr[256:384] = y
    out[256:320] = False
    out[320:384] = np.arange(64) % 2 == 0
    batches = [_plain_rows(0, 200).tobytes(), _rows(addr, out, _t(1)).tobytes()]
    wins = _check(oracle, batches, [(0, 0), (1, 0)])
    assert {"name": "20.%d.%d.%d" % (y >> 16 & 255, y >> 8 & 255, y & 255), "estimate": 128} in wins[1]["packets"]["top_ipv4"]


@pytest.mark.parametrize("where", ["first_group", "last_group", "middle_group"])
@pytest.mark.parametrize("what", ["dns", "vlan", "ipv6"])
def test_wrong_guess_partial_combine(oracle, what, where):
    """five batches in one window; batch 3 (fused on the guess) holds one record the short chain
    cannot take, so only that group's workgroup skips its combine: the others have listed their
    ranges when the merge's guard stops it and the regular chain combines the batch again. Batch
    4 runs the regular chain, batch 5 is fused again. No top_ipv4 estimate may count twice."""
    c = _cus()
    n = 3 * c * 64
    k = {"first_group": 5, "last_group": n - 3, "middle_group": 192 * (c // 2) + 100}[where]
    x = int(_remote(7001))
    sub = {"dns": _rec_dns(int(_remote(7002)), ME, _t(2, k), 77), "vlan": _rec_vlan(x, ME, _t(2, k)), "ipv6": _rec_v6(9, _t(2, k))}[what]
    rows = [_plain_rows(b, n) for b in range(5)]
    batches = [r.tobytes() for r in rows]
    batches[2] = _with(rows[2], {k: sub})
    wins = _check(oracle, batches, [(0, 0), (1, 0), (2, 1), (2, 1), (3, 1)])
    assert wins[4]["packets"]["events"] == 5 * n
    if what == "ipv6":
        assert wins[4]["packets"]["top_ipv6"] == [{"name": "2001:db8::9", "estimate": 1}]


def test_spill_inside_the_fused_kernel(oracle):
    """groups of 192 k records, every one a key of its own: k = 89 is the smallest with more than
    17K keys a group (17,088), past the compact table's 16384 slots and below 65,536 records. The
    addresses are n / 3, three times over (addresses seen once each leave top_ipv4 to the purges:
    test_gpu_combine_compact.test_group_past_the_16bit_bounds)."""
    c = _cus()
    k = -(-17000 // 192)
    n = 3 * c * 64 * k
    i = np.arange(n, dtype=np.int64)
    big = _rows((20 << 24) + 1 + i % (n // 3), i % 3 == 0, _t(1), step_us=1).tobytes()
    assert 192 * k >= 17000 and 192 * k < 65536 and n // 3 > 192 * k
    batches = [_plain_rows(0, 200).tobytes(), big]
    _check(oracle, batches, [(0, 0), (1, 0)])


def test_generic_table_in_a_fused_launch(oracle):
    """PV_CB_COMPACT=0 with PV_CB_FAN=3: the fused kernel's workgroups run the generic table in place"""
    n = 3 * _cus() * 64 * 2 - 37
    batches = [_plain_rows(b, n).tobytes() for b in range(2)]
    _check(oracle, batches, [(0, 0), (1, 0)], env={"PV_CB_COMPACT": "0", "PV_CB_FAN": "3"})


def _without_geo(w):
    w = dict(w)
    w["packets"] = {k: v for k, v in w["packets"].items() if k not in ("top_geoLoc", "top_ASN")}
    return w


NOT_FUSED = {"75_ranges": (4800, {}, {}, None),
             "net_v2": (None, {"net2_config": {}}, {"net2_groups": 31}, None),
             "geoip": (None, {"geo_city_db": os.path.join(GOLD, "GeoIP2-City-Test.mmdb"),
                              "geo_asn_db": os.path.join(GOLD, "GeoIP2-ISP-Test.mmdb")}, {}, _without_geo)}


@pytest.mark.parametrize("what", list(NOT_FUSED))
def test_not_fused(oracle, what):
    """too few ranges for a group a CU; Net v2 and GeoIP counting never start the short chain.
    (PV_FUSE_PLAIN=0 is the second run of every test here.)"""
    n, kw, okw, strip = NOT_FUSED[what]
    n = n or 3 * _cus() * 64
    batches = [_plain_rows(b, n).tobytes() for b in range(3)]
    _check(oracle, batches, [(0, 0)] * 3, okw=okw, strip=strip, **kw)


def test_stamped_batches_stay_unfused(oracle):
    """pv_set_kernel_timing(2): every second batch is dispatch-stamped and keeps the two launches,
    its stamps around the Net pass alone: the stamped time is the one the same context measures
    with PV_FUSE_PLAIN=0: both are the same kernel over the same records, and a factor of two
    either way covers the run-to-run spread of a kernel of some ten microseconds"""
    n = 3 * _cus() * 64 * 2 - 37
    batches = [_plain_rows(b, n).tobytes() for b in range(6)]
    wins, stats, (ms, launches) = _run(batches, timing=2)
    wins0, stats0, (ms0, launches0) = _run(batches, fuse="0", timing=2)
    # batches 1, 3, 5 are stamped (and batch 1 has no guess yet); 2, 4 and 6 run fused
    assert stats == [(0, 0), (1, 0), (1, 0), (2, 0), (2, 0), (3, 0)], stats
    assert stats0 == [(0, 0)] * 6
    assert launches == launches0 == 3
    print("stamped Net pass, ms over 3 launches: fused context %.4f, PV_FUSE_PLAIN=0 %.4f" % (ms, ms0))
    assert 0 < ms < 2 * ms0 and ms0 < 2 * ms, (ms, ms0)
    assert wins == wins0
    assert diff(wins[5], _ref(oracle, batches, 6)) is None
