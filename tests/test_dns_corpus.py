"""Conditions on the inputs of the device decode fuzz (tests/dns_corpus.py), from the builder's own
arithmetic and the oracle alone: the corpus reaches every cell of the two window edges, the tile
shapes hold the long messages their names say, enough messages decode to a name, and no top list
of the oracle is cut at the topn_count the GPU test uses. No product code runs here."""
import ctypes

import pytest

from tests import dns_corpus as dc
from tests.test_decoder_fuzz import oracle_fns


@pytest.fixture(scope="module")
def families():
    return dc.family_batches()


@pytest.fixture(scope="module")
def shapes():
    return dc.shape_batches()


@pytest.fixture(scope="module")
def every_batch(families, shapes):
    mixed, rev = dc.mixed_batches()
    return list(families.values()) + [mixed, rev, dc.large_batch()] + [b for b, _ in shapes.values()]


def name_end(oracle_lib, msg):
    """encoded length of the first question name as the oracle walks it (0: none)"""
    out, n = ctypes.create_string_buffer(4096), ctypes.c_uint32()
    return oracle_lib.pvo_decode_qname(msg + bytes(16), len(msg), out, ctypes.byref(n))


def test_message_end_cells(families):
    """every residue of moff & 15 occurs with a message whose end, measured from its window base,
    falls in each of <= 120, 121..124, 125..128 and > 128: 64 cells around the `fits` edge"""
    cells = {}
    for b in families.values():
        for r in b.recs:
            if r.dns:
                end = (r.moff & 15) + max(r.mlen, r.mcap)
                cls = 0 if end <= 120 else 1 if end <= 124 else 2 if end <= 128 else 3
                cells[(r.moff & 15, cls)] = cells.get((r.moff & 15, cls), 0) + 1
                assert dc.fits(r.moff, r.mlen, r.mcap) == (cls < 2)
    print("message-end cells (residue, class): min %d, max %d records" % (min(cells.values()), max(cells.values())))
    assert len(cells) == 64, sorted(set((m, c) for m in range(16) for c in range(4)) - set(cells))


def test_name_end_cells(families, oracle):
    """the same for the end of the question name measured from the record's 16-byte aligned start,
    against the names kernel's 192-byte window: <= 184, 185..192, 193..200 and > 200"""
    lib = oracle_fns(oracle)
    cells = {}
    for b in families.values():
        for r in b.recs:
            if not r.dns or r.mlen < 13:
                continue
            nl = name_end(lib, r.msg[: r.mlen])
            if nl == 0:
                continue
            end = (r.roff & 15) + (r.moff - r.roff) + 12 + nl
            cls = 0 if end <= 184 else 1 if end <= 192 else 2 if end <= 200 else 3
            cells[(r.roff & 15, cls)] = cells.get((r.roff & 15, cls), 0) + 1
    print("name-end cells (residue, class): min %d, max %d records" % (min(cells.values()), max(cells.values())))
    assert len(cells) == 64, sorted(set((m, c) for m in range(16) for c in range(4)) - set(cells))


def test_tile_shapes_hold_their_long_messages(shapes):
    """the `fits` rule restated: the messages that go to the long list are the ones each shape names"""
    want = {"n1": 1, "n63": 13, "n64": 13, "n65": 13, "n129": 26, "all_long": 64, "one_long_first": 1, "one_long_last": 1,
            "long_tile": 64}
    count = {"n1": 1, "n63": 63, "n64": 64, "n65": 65, "n129": 129, "all_long": 64, "one_long_first": 64, "one_long_last": 64,
             "long_tile": 198}
    assert set(shapes) == set(want)
    for name, (b, long_idx) in shapes.items():
        assert all(r.dns for r in b.recs) and len(b.recs) == count[name]
        got = [i for i, r in enumerate(b.recs) if not dc.fits(r.moff, r.mlen, r.mcap)]
        assert got == long_idx and len(got) == want[name], (name, got)
        # a long message is at least 125 bytes from its window base, as the issue words it
        assert all((b.recs[i].moff & 15) + b.recs[i].mlen >= 125 for i in got)
    assert shapes["one_long_first"][1] == [0] and shapes["one_long_last"][1] == [63]
    assert shapes["long_tile"][1] == list(range(64, 128))


def test_families_decode_to_names(families, oracle):
    """at least 60 % of each structured family's messages parse with a question and a non-empty name;
    in junk both outcomes occur"""
    lib = oracle_fns(oracle)
    ok, hq, qt = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint32()
    out, n = ctypes.create_string_buffer(4096), ctypes.c_uint32()
    for fam, b in families.items():
        named = total = 0
        for r in b.recs:
            if not r.dns or r.mlen < 12:
                total += r.dns
                continue
            msg = r.msg[: r.mlen]
            lib.pvo_dns_parse(msg + bytes(16), len(msg), ctypes.byref(ok), ctypes.byref(hq), ctypes.byref(qt))
            nl = lib.pvo_decode_qname(msg + bytes(16), len(msg), out, ctypes.byref(n))
            named += bool(ok.value and hq.value and nl and n.value)
            total += 1
        print(f"{fam}: {total} messages, {named / total:.1%} with a question and a name")
        if fam == "junk":
            assert 0 < named < total
        else:
            assert named / total >= 0.6, (fam, named, total)


def test_builder_places_messages_where_the_oracle_finds_them(every_batch, oracle):
    """moff and mlen of every record against the oracle's frame walk (parse_packet): the UDP layer at
    moff - 8, its length mlen + 8, bounded by the IP length and by the capture; records the builder
    calls no DNS message have no whole UDP header"""
    from tests.test_parse_fuzz import oracle_rows
    cut = 0
    for b in every_batch:
        rows = oracle_rows(oracle, b.blob, len(b.recs), 1, dc.HOST)
        for r, row in zip(b.recs, rows):
            if r.dns:
                assert (row[1], row[8], row[9]) == (17, r.moff - r.roff - 16 - 8, r.mlen + 8), (b.name, r, row.tolist())
                assert r.mlen <= r.mcap
                cut += r.mlen < len(r.msg)
            else:
                assert row[1] == 0, (b.name, r, row.tolist())
    print(f"{cut} messages cut by the capture (mlen below the UDP length)")
    assert cut > 100


def test_waves_batch_fills_every_range():
    """on 256 CUs with one range a CU: ten tiles of 64 DNS messages a range, more than a tile of them
    long and more than a tile not (the GPU test asserts the same for the device it runs on)"""
    b = dc.waves_batch(256)
    ranges, wt = dc.pass_partition(len(b.recs), 256, 1)
    assert (ranges, wt) == (256, 10) and all(r.dns for r in b.recs)
    assert dc.pass_partition(6822, 256, 3) == (107, 1)  # the large batch: a tile a range, one wave decodes
    longs = [sum(not dc.fits(r.moff, r.mlen, r.mcap) for r in b.recs[k * 640:(k + 1) * 640]) for k in range(ranges)]
    print(f"waves: {len(b.recs)} records, long messages a range {min(longs)}..{max(longs)}")
    assert 64 < min(longs) and max(longs) < 640 - 64


def test_batch_sizes(families, every_batch):
    for fam, b in families.items():
        assert 300 <= len(b.recs) <= 600, (fam, len(b.recs))
    large = [b for b in every_batch if b.name == "large"][0]
    assert 5000 <= len(large.recs) <= 8000
    mixed, rev = [b for b in every_batch if b.name.startswith("mixed")]
    assert [r.msg for r in mixed.recs] == [r.msg for r in rev.recs][::-1]


@pytest.mark.parametrize("case", ["v1", "v2"])
def test_oracle_top_lists_are_whole(every_batch, oracle, case):
    """with the topn_count the GPU test uses, every top list of every batch is strictly shorter than
    it: nothing is cut, so a failing GPU run can list the names each side has alone"""
    longest = 0

    def walk(v, n):
        nonlocal longest
        if isinstance(v, dict):
            for x in v.values():
                walk(x, n)
        elif isinstance(v, list):
            assert len(v) < n
            longest = max(longest, len(v))

    for b in every_batch:
        n = dc.topn_for(b)
        assert n > len(b.recs)
        walk(oracle.run_bytes(dc.pcap_of(b), host_spec=dc.HOST, num_periods=1, window=1, topn_count=n, **dc.CASES[case][1]), n)
    print(f"{case}: {len(every_batch)} batches, the longest top list has {longest} entries")
