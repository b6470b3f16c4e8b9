"""Device decode fuzz: the DNS corpus of tests/dns_corpus.py (messages and names placed across the
edges of the DNS pass's 128-byte LDS window and the names kernels' 192-byte window, compression
pointers, ECS records around the edge, long lists of every tile shape) through the DNS pass, its long
pass, pv_dns_suffix, pv_dns_ecs, pv_topn_names / pv_topn_names_sfx and pv_dns_tcp, bit-exact against
the oracle on the same pcap bytes. topn_count is above every batch's record count, so the top lists
are whole and a mismatch names the exact messages.

What the inputs reach (every cell of both edges, the long messages of each tile shape) is asserted on
the CPU in tests/test_dns_corpus.py. Path guards: pv_chain_stats must show that every batch ran the
regular chain (the DNS stage and the names kernel; the library counts no single DNS kernel, and which
of them a chain runs is the host's function of the config alone); each case's oracle result must
differ from the plain one in the way the case's path implies (and equal the GPU's); the TCP case
must count every message as TCP; the waves case asserts the tiles a range the device's partition
gives it.

Not reached here: the names kernels' second loop iteration (an entry decoded while the next one's
window is in flight) needs more new names in a batch than the kernel has lanes, about 131,000 on
256 CUs; these batches give each lane at most one entry."""
import json
import random

import pytest

import pktvisor_amd as pa
from tests import dns_corpus as dc
from tests import parse_corpus as pc
from tests.test_gpu_parity import diff

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- batches, built once
@pytest.fixture(scope="module")
def batches():
    fam = dc.family_batches()
    mixed, rev = dc.mixed_batches()
    small = list(fam.values()) + [b for b, _ in dc.shape_batches().values()]
    return {"small": small, "big": [mixed, rev, dc.large_batch()]}


def name_lists(v, path=""):
    """{path: [names]} of every top list in a window"""
    out = {}
    if isinstance(v, dict):
        for k, x in v.items():
            out.update(name_lists(x, f"{path}.{k}"))
    elif isinstance(v, list) and v and isinstance(v[0], dict) and "name" in v[0]:
        out[path] = [e["name"] for e in v]
    return out


def explain(gpu, ref):
    """the first differing path, then per top list the names only one side has (the lists are whole)"""
    lines = [diff(gpu, ref) or "no difference"]
    a, b = name_lists(gpu), name_lists(ref)
    for path in sorted(set(a) | set(b)):
        ga, rb = set(a.get(path, [])), set(b.get(path, []))
        if ga != rb:
            lines.append(f"{path}: only the oracle has {sorted(rb - ga)[:40]}; only the GPU has {sorted(ga - rb)[:40]}")
    return "\n".join(lines)


def run_gpu(h, recs: bytes):
    h.reset()
    h.chain_stats(reset=True)
    h.process_host(recs)
    h.set_end_tstamp(*pa.last_record_ts(recs, pa.RecordIndex(recs)))
    out = {"1m": h.window_json(0)}
    # every batch holds UDP DNS messages: each ran the regular chain (DNS stage, top-N, names kernel),
    # straight away or after a short-chain start that fell back
    short, fell_back, _, regular = h.chain_stats(reset=True)
    assert regular + fell_back >= 1 and short == fell_back, (short, fell_back, regular)
    return out


def run_oracle(oracle, batch_pcap, topn, okw):
    return oracle.run_bytes(batch_pcap, host_spec=dc.HOST, num_periods=1, window=1, topn_count=topn, **okw)


def table_log2(big):
    return 15 if big else 13


def context(case, big, max_records=1 << 13):
    """family and tile-shape batches: topn_count 1024, tables of 2^13 slots (more than twice the 600
    keys a batch can give one table); the mixed and large ones: 8192 and 2^15 (at most 6,900 keys);
    no_purge() holds each batch to it"""
    return pa.PvHandlers(host_spec=dc.HOST, num_periods=1, topn_count=8192 if big else 1024, table_log2=table_log2(big),
                         max_records=max_records, net_config={}, **dc.CASES[case][0])


def no_purge(ref, big, batch):
    """every table holds more than twice the batch's distinct keys (the oracle's lists are whole, so
    the longest one counts them), so no purge runs"""
    keys = max([len(v) for v in name_lists(ref).values()] + [0])
    assert 2 * keys < 1 << table_log2(big), (batch.name, keys)


def dns_of(w):
    return w["1m"]["dns"]


def guard(case, ref, plain, batch):
    """the case's path shows in the oracle's result for this batch (and the GPU's equals it)"""
    d, p = dns_of(ref), dns_of(plain)
    if case in ("v1", "v2"):
        assert name_lists(d), batch.name  # names came back: the names kernel decoded them
    elif case == "v1_psl":
        assert d["top_qname2"] != p["top_qname2"], batch.name  # listed suffixes moved the aggregation
    else:
        assert d != p, batch.name
        if case.startswith("v1"):
            # the filter took some messages and left others (edge_name has no RRSIG answer: all taken)
            f, n = d["wire_packets"]["filtered"], d["wire_packets"]["events"]
            assert 0 < f and (f < n or (case, batch.name) == ("v1_dnssec", "edge_name")), (batch.name, f, n)


GUARDED = ("mixed", "mixed_reversed", "large", "rcode", "edge_name")  # batches every case's path shows in


@pytest.mark.parametrize("case", list(dc.CASES))
def test_corpus_matches_oracle(oracle, batches, case):
    okw = dc.CASES[case][1]
    plain_kw = dc.CASES["v2" if case.startswith("v2") else "v1"][1]
    guarded = 0
    for big in (False, True):
        h = context(case, big)
        try:
            for b in batches["big" if big else "small"]:
                topn = dc.topn_for(b)
                assert topn == (8192 if big else 1024)
                pcap = dc.pcap_of(b)
                ref = run_oracle(oracle, pcap, topn, okw)
                no_purge(ref, big, b)
                gpu = run_gpu(h, b.blob)
                assert diff(gpu, ref) is None, f"{case} / {b.name}:\n" + explain(gpu, ref)
                if b.name in GUARDED:
                    guard(case, ref, run_oracle(oracle, pcap, topn, plain_kw), b)
                    guarded += 1
        finally:
            h.close()
    assert guarded == len(GUARDED)


def test_mixed_order_guard(oracle, batches):
    """the same records forward and reversed both equal the oracle, and the two results hold the same
    names: no lane's decode depends on its neighbours' windows"""
    mixed, rev = batches["big"][:2]
    okw = dc.CASES["v1"][1]
    h = context("v1", True)
    try:
        out = []
        for b in (mixed, rev):
            ref = run_oracle(oracle, dc.pcap_of(b), 8192, okw)
            gpu = run_gpu(h, b.blob)
            assert diff(gpu, ref) is None, f"{b.name}:\n" + explain(gpu, ref)
            out.append(gpu)
    finally:
        h.close()
    a, b = name_lists(out[0]), name_lists(out[1])
    assert set(a) == set(b)
    for path in a:
        if "slow" not in path:  # (the slow-transaction threshold follows arrival order)
            assert sorted(a[path]) == sorted(b[path]), path


# ---------------------------------------------------------------- every wave of a workgroup
@pytest.fixture(scope="module")
def waves():
    """(batch, its pcap, ranges, tiles a range) for this device with one range a CU"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b = dc.waves_batch(min(cus, 1024))
    ranges, wt = dc.pass_partition(len(b.recs), cus, 1)
    return b, dc.pcap_of(b), ranges, wt


@pytest.mark.parametrize("case", ["v1", "v1_psl", "v1_qtype", "v2"])
def test_every_wave_of_a_workgroup(oracle, monkeypatch, waves, case):
    """The batches above give a range of the DNS pass one tile, which its first wave decodes. Here
    every range has ten tiles of 64 DNS messages (one range a CU, PV_NET_WGCU=1): all eight waves
    stage windows next to each other and decode, two of them a second tile behind the descriptor and
    window prefetch, and the range's long list fills several tiles of the long pass. The pass of each
    kind: plain, with suffix sizes, with the filter block, v2."""
    b, pcap, ranges, wt = waves
    assert wt >= 10 and all(r.dns for r in b.recs) and len(b.recs) == ranges * wt * 64
    for k in range(ranges):
        n_long = sum(not dc.fits(r.moff, r.mlen, r.mcap) for r in b.recs[k * wt * 64:(k + 1) * wt * 64])
        assert 64 < n_long < wt * 64 - 64, (k, n_long)  # more than a tile in the long pass, more than a tile not
    monkeypatch.setenv("PV_NET_WGCU", "1")
    ref = run_oracle(oracle, pcap, 8192, dc.CASES[case][1])
    no_purge(ref, True, b)
    assert max(len(v) for v in name_lists(ref).values()) < 8192
    h = context(case, True, max_records=1 << 18)
    try:
        gpu = run_gpu(h, b.blob)
    finally:
        h.close()
    assert diff(gpu, ref) is None, f"{case} / waves:\n" + explain(gpu, ref)


# ---------------------------------------------------------------- DNS over TCP
def tcp_messages():
    """about 300 of the corpus's messages, some from every family, that a TCP length prefix can carry"""
    rng = random.Random(17)
    per = {}
    for fam, m in dc.all_messages():
        if m:
            per.setdefault(fam, []).append(m)
    out = []
    for fam in sorted(per):
        rng.shuffle(per[fam])
        out += per[fam][:40]
    rng.shuffle(out)
    return out


def test_tcp_messages_match_oracle(oracle):
    """each message in a TCP flow of its own (SYN, length prefix and message in one or two segments,
    FIN): pv_dns_tcp's flat accessor over the message arena and the names of message records; once as
    one batch, once as batches of 1..200 records"""
    msgs = tcp_messages()
    assert 250 <= len(msgs) <= 400
    recs = dc.tcp_records(msgs)
    blob = b"".join(recs)
    pcap = pc.pcap(recs)
    ref = run_oracle(oracle, pcap, 1024, dc.CASES["v1"][1])
    no_purge(ref, False, dc.Batch("tcp", blob, []))
    w = dns_of(ref)["wire_packets"]
    print("TCP case: %d messages in %d records, the oracle counts %d TCP DNS events" % (len(msgs), len(recs), w["tcp"]))
    # every message of at least the reference's minimum DNS-over-TCP size (17 bytes) is an event; none travels by UDP
    assert w["udp"] == 0 and w["tcp"] == sum(len(m) >= 17 for m in msgs) > 250 and name_lists(dns_of(ref))
    rng = random.Random(5)
    for split in (False, True):
        h = context("v1", False)
        try:
            h.reset()
            if split:
                i = 0
                while i < len(recs):
                    j = min(len(recs), i + rng.randrange(1, 201))
                    h.process_host(b"".join(recs[i:j]))
                    i = j
            else:
                h.process_host(blob)
            h.set_end_tstamp(*pa.last_record_ts(blob, pa.RecordIndex(blob)))
            gpu = {"1m": h.window_json(0)}
            stats = h.chain_stats()
            assert stats[3] + stats[1] >= 1, stats  # the regular chain ran: pv_dns_tcp's messages behind its DNS stage
        finally:
            h.close()
        assert diff(gpu, ref) is None, ("batches of 1..200" if split else "one batch") + ":\n" + explain(gpu, ref)


def test_explain_lists_the_names_each_side_has_alone():
    a = {"1m": {"dns": {"top_qname2": [{"name": "x", "estimate": 1}, {"name": "y", "estimate": 1}]}}}
    b = json.loads(json.dumps(a))
    b["1m"]["dns"]["top_qname2"][1]["name"] = "z"
    text = explain(a, b)
    assert "only the oracle has ['z']" in text and "only the GPU has ['y']" in text and ".1m.dns.top_qname2[1].name" in text
