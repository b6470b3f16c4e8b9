"""The adversarial frame corpus of tests/parse_corpus.py (the CPU fuzz's generator, with DNS queries
and BGP / DHCP messages as L4 payloads) through every Net-pass path and the DHCP and BGP scans.

Net: one worker process per path (tests/parse_path_worker.py; PV_NET_KERNEL is read once per
process), one after another. Each asserts the kernel the library launched and compares every batch
bit-exactly with the oracle: one batch a frame family, a mixed batch in both orders (an outcome
that depends on a neighbour's bytes shows), and the lean passes' tile shapes.
DHCP / BGP: the same L2/L3 shapes with UDP/67-68 and TCP/179 behind them against the Python models,
which exercises the scans' header-window classifiers and their fall-back to parse_record."""
import json
import os
import random
import subprocess
import sys

import pytest

from tests import bgp_cases as bc
from tests import dhcp_cases as dc
from tests import parse_corpus as pc
from tests.parse_path_worker import CASES, T0

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", list(CASES))
def test_net_path_matches_oracle(case):
    env = dict(os.environ)
    env.pop("PV_NET_KERNEL", None)
    if CASES[case].get("force"):
        env["PV_NET_KERNEL"] = CASES[case]["force"]
    r = subprocess.run([sys.executable, "-m", "tests.parse_path_worker", case], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    res = [json.loads(line[7:]) for line in r.stdout.splitlines() if line.startswith("RESULT ")]
    names = [x["batch"] for x in res]
    assert {"ipv4", "ipv6", "tunnel", "l4", "mixed", "mixed_reversed"} <= set(names), names
    if CASES[case].get("linktype", 1) == 1:
        assert {"l2", "bounds", "tile_n1", "tile_n63", "tile_n64", "tile_n65", "tile_n257", "all_general", "general_first",
                "general_last", "general_tile"} <= set(names), names
    for x in res:
        print(case, x)
    assert [x["kernel"] for x in res] == [CASES[case]["kernel"]] * len(res), [(x["batch"], x["kernel"]) for x in res]
    assert [(x["batch"], x["diff"]) for x in res if x["diff"]] == []
    by = {x["batch"]: x for x in res}
    # the inputs are not vacuous: the family batches carry both protocols past the walk
    for fam in ("ipv4", "ipv6", "tunnel", "l4", "mixed"):
        assert by[fam]["udp"] > 20 and by[fam]["tcp"] > 20, by[fam]
    if "bounds" in by:
        # 6..11 extension headers and 2..5 nested IPv4 headers reach their UDP layer, 6 nested do not
        assert (by["bounds"]["n"], by["bounds"]["udp"]) == (11, 10), by["bounds"]


# ---------------------------------------------------------------- DHCP and BGP scans
def bgp_l4(rng, proto, tag):
    if proto == 6:
        return bc.tcp(bc.bgp_msg(4), 40000 + rng.randrange(0, 2000), 179, rng.getrandbits(32))
    return pc.dns_l4(rng, 17, tag)


def dhcp_l4(rng, proto, tag):
    if proto == 17:
        return dc.udp(dc.bootp(3, rng.getrandbits(32), opts=[(12, tag.encode())]), 68, 67)
    return pc.dns_l4(rng, 6, tag)


def shape_batches(l4gen, proto, linktype):
    """[(name, records)]: one batch a frame family and the bounds batch, every L4 layer from l4gen"""
    rng = random.Random(500 + proto + linktype)
    fams = ("l2", "ipv4", "ipv6", "tunnel", "l4") if linktype == 1 else ("ipv4", "ipv6", "tunnel")
    out = []
    for fam in fams:
        frames = pc.frames_of(rng, fam, 200, l4gen, linktype=linktype, maxlb=1)
        out.append((fam, b"".join(pc.record(f, sec=T0, usec=i) for i, f in enumerate(frames))))
    if linktype == 1:
        frames = [pc.ext_chain_frame(n, l4gen(rng, proto, "ext%d" % n), proto) for n in range(6, 12)]
        frames += [pc.nested_v4_frame(k, l4gen(rng, proto, "nest%d" % k), proto) for k in range(2, 7)]
        out.append(("bounds", b"".join(pc.record(f, sec=T0, usec=i) for i, f in enumerate(frames))))
    return out


@pytest.mark.parametrize("linktype", [1, 113, 101])
def test_bgp_scan_over_the_frame_shapes(linktype):
    from tests.test_gpu_bgp import gpu as bgp_run
    for name, recs in shape_batches(bgp_l4, 6, linktype):
        got, want = bgp_run([recs], linktype=linktype, num_periods=1)
        print(linktype, name, want["wire_packets"])
        assert got == want, name
        # 11 frames of the bounds batch, the one with six IPv4 headers has no TCP layer: ten KEEPALIVEs
        n = want["wire_packets"]["keepalive"]
        assert (n == 10) if name == "bounds" else (n > 10), (name, n)


@pytest.mark.parametrize("linktype", [1, 113, 101])
def test_dhcp_scan_over_the_frame_shapes(linktype):
    from tests.test_gpu_dhcp import gpu as dhcp_run
    for name, recs in shape_batches(dhcp_l4, 17, linktype):
        got, want = dhcp_run([recs], linktype=linktype, num_periods=1)
        print(linktype, name, want["wire_packets"])
        assert got == want, name
        n = want["wire_packets"]["request"]
        assert (n == 10) if name == "bounds" else (n > 10), (name, n)
