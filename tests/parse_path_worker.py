"""One Net-pass path over the adversarial frame corpus (tests/parse_corpus.py), in a process of its
own: PV_NET_KERNEL is read once per process, so tests/test_gpu_parse_paths.py starts one worker per
case, one after another.

usage: [PV_NET_KERNEL=<variant>] python -m tests.parse_path_worker <case>
Every batch runs in a fresh context and is compared bit-exactly with the oracle over the same pcap
(one period). Prints one line "RESULT {json}" per batch with the kernel the library launched and
the first differing path (null when equal); exits 0 when the case ran, whatever it found."""
import json
import random
import sys

from tests import parse_corpus as pc

T0 = 1_700_000_000
DNS2_ALL = ["cardinality", "counters", "quantiles", "top_ecs", "top_qtypes", "top_rcodes", "top_size", "top_qnames",
            "top_ports", "xact_times"]
# case -> the kernel it must launch, the forced variant, link type, host spec, handler and oracle keywords
CASES = {
    "default": dict(kernel="pv_net_kernel_reg_tc"),
    "lean_no_top_ips": dict(kernel="pv_net_kernel_reg", hkw={"net_groups": 3}, okw={"net_groups": 3}),  # counters | cardinality
    "span": dict(kernel="pv_net_kernel_span", force="span"),
    "ns": dict(kernel="pv_net_kernel_ns", force="ns"),
    "general": dict(kernel="pv_net_kernel", force="general"),
    "five_v4_subnets": dict(kernel="pv_net_kernel_ns", spec=pc.FIVE_V4_SPEC),
    "linktype_113": dict(kernel="pv_net_kernel_ns", linktype=113),
    "linktype_101": dict(kernel="pv_net_kernel_ns", linktype=101),
    "net2_dns2": dict(kernel="pv_net_kernel_reg_tc", hkw={"net2_config": {}, "dns2_config": {"enable": DNS2_ALL}},
                      okw={"net2_groups": 31, "dns2_groups": 0x3ff}),
}
MAXLEN = 184  # a record of at most 200 bytes


def stamp(frames):
    return [pc.record(f, sec=T0, usec=i) for i, f in enumerate(frames)]


def plain(rng, n):
    """Ethernet + IPv4 without options + a UDP DNS query: the lean passes' fast path"""
    return [pc.eth(rng, pc.v4hdr(rng, pc.dns_l4(rng, 17, "plain"), 17), 0x0800) for _ in range(n)]


def general(rng, n):
    """frames the fast path declines: IPv6 chains, and IPv4 behind a VLAN tag or with options"""
    out = pc.frames_of(rng, "ipv6", n - n // 3, pc.dns_l4, maxlen=MAXLEN, maxlb=1)
    for i in range(n // 3):
        v4 = pc.v4hdr(rng, pc.dns_l4(rng, 17, "gen"), 17, ihl=5 + i % 2)
        out.append(pc.eth(rng, v4, 0x0800, [0x8100] if i % 2 == 0 else ()))
    rng.shuffle(out)
    return out


def batches(linktype):
    """[(name, frames)], seeded: one batch a family, the mixed batch both ways, the tile shapes"""
    rng = random.Random(77 + linktype)
    fams = ("l2", "ipv4", "ipv6", "tunnel", "l4") if linktype == 1 else ("ipv4", "ipv6", "tunnel", "l4")
    gen = lambda fam, n: pc.frames_of(rng, fam, n, pc.dns_l4, linktype=linktype, maxlen=MAXLEN, maxlb=1)  # noqa: E731
    out = [(fam, gen(fam, 400)) for fam in fams]
    if linktype == 1:
        # the frames that separated the two walks, with a DNS query behind them
        q = lambda tag: pc.dns_l4(rng, 17, tag)  # noqa: E731
        out.append(("bounds", [pc.ext_chain_frame(n, q("ext%d" % n), 17) for n in range(6, 12)]
                    + [pc.nested_v4_frame(k, q("nest%d" % k), 17) for k in range(2, 7)]))
    mixed = []
    for fam in fams:
        mixed += gen(fam, 3000 // len(fams))
    rng.shuffle(mixed)
    out += [("mixed", mixed), ("mixed_reversed", mixed[::-1])]
    if linktype == 1:
        for n in (1, 63, 64, 65, 257):
            out.append(("tile_n%d" % n, [rng.choice(mixed) for _ in range(n)]))
        out.append(("all_general", general(rng, 130)))
        out.append(("general_first", general(rng, 1) + plain(rng, 199)))
        out.append(("general_last", plain(rng, 199) + general(rng, 1)))
        out.append(("general_tile", plain(rng, 64) + general(rng, 64) + plain(rng, 70)))
    return out


def main():
    case = CASES[sys.argv[1]]
    import torch
    if torch.cuda.device_count() > 0:
        torch.cuda.init()  # torch's HIP runtime first (tests/conftest.py)
    import pktvisor_amd as pa
    from tests.oracle_ctypes import load as load_oracle
    from tests.test_gpu_parity import diff
    oracle = load_oracle()
    linktype, spec = case.get("linktype", 1), case.get("spec", pc.DEFAULT_SPEC)
    for name, frames in batches(linktype):
        recs = stamp(frames)
        blob = b"".join(recs)
        h = pa.PvHandlers(host_spec=spec, num_periods=1, linktype=linktype, max_records=len(recs), **case.get("hkw", {}))
        try:
            h.process_host(blob)
            h.set_end_tstamp(*pa.last_record_ts(blob, pa.RecordIndex(blob)))
            kernel = h.net_kernel_name()
            gpu = h.window_json(0)
        finally:
            h.close()
        ref = oracle.run_bytes(pc.pcap(recs, linktype), host_spec=spec, num_periods=1, window=1, **case.get("okw", {}))["1m"]
        print("RESULT", json.dumps({"batch": name, "n": len(recs), "kernel": kernel, "diff": diff(gpu, ref),
                                    "udp": ref["packets"]["udp"], "tcp": ref["packets"]["tcp"]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
