"""The cost of the DNS v1 handler's geo half (pv_set_dns_geo) on a device-resident capture of
DNS queries that all carry an EDNS Client Subnet, drawn Zipf-like from about 1,000 subnets inside
and outside the two test databases: the step time with top_ecs on and no database (the path every
context took before the switch existed), with both databases counted, and with both *_notfound
filters on; and, by HIP events through the kernel-timing switch, pv_dns_geo_verdict, the DNS pass,
pv_dns_ecs and pv_dns_ecs_geo of the same runs (DESIGN; profiles/dns_geo/measure.json).
Usage: python tools/dns_geo_measure.py [QUERIES [OUT.json]]"""
import ipaddress
import json
import os
import statistics
import struct
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pktvisor_amd as pa  # noqa: E402
from tests import dns_geo_cases as C  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else None
STEPS, WARMUP = 10, 2
GOLD = os.path.join(ROOT, "tests", "golden")
CITY, ISP = os.path.join(GOLD, "GeoIP2-City-Test.mmdb"), os.path.join(GOLD, "GeoIP2-ISP-Test.mmdb")
V4_NETS = ["89.160.20.0", "81.2.69.0", "216.160.83.0", "1.128.0.0", "12.81.92.0", "8.8.8.0", "6.6.6.0", "203.0.113.0"]
V6_NETS = ["2a02:dac0::", "2001:218::", "2001:1700::", "2001:db8::", "2001:470:1f0b::"]


def subnets(rng, n=1000):
    out = []
    for k in range(n):
        if k % 10 < 7:
            base = int(ipaddress.ip_address(V4_NETS[k % len(V4_NETS)]))
            out.append((1, ipaddress.ip_address(base + int(rng.integers(0, 256))).packed[:3 + k % 2]))
        else:
            base = ipaddress.ip_address(V6_NETS[k % len(V6_NETS)]).packed
            out.append((2, base[:4] + bytes(rng.integers(0, 256, 4, dtype=np.uint8))))
    return out


def capture(n, seed=7):
    rng = np.random.default_rng(seed)
    subs = subnets(rng)
    frames = [C.ecs_query(k, s, six=k % 3 == 2) for k, s in enumerate(subs)]
    pick = np.minimum(rng.zipf(1.3, n) - 1, len(subs) - 1)
    parts = []
    for i, k in enumerate(pick):
        fr = frames[k]
        parts.append(struct.pack("<IIII", C.T0 + i // 1000000, i % 1000000, len(fr), len(fr)))
        parts.append(fr)
    return b"".join(parts), len(set(pick.tolist()))


def phase(d_recs, d_offs, idx, geo: bool, filters: bool):
    kw = dict(geo_city_db=CITY, geo_asn_db=ISP, dns_geo=True) if geo else {}
    dcfg = {"enable": ["top_ecs"]}
    if filters:
        dcfg.update(geoloc_notfound=True, asn_notfound=True)
    h = pa.PvHandlers(host_spec=C.HOST, num_periods=5, max_records=N, device=0, net_config={}, dns_config=dcfg, **kw)
    try:
        def step():
            h.process_device(d_recs.data_ptr(), d_offs.data_ptr(), idx)
            h.synchronize()
        for _ in range(WARMUP):
            h.reset()
            step()
        out = {}
        for name, every in (("unstamped", 0), ("stamped", 1)):
            h.set_kernel_timing(every)
            if geo:
                h.dns_geo_timing(reset=True)
            ms = []
            for _ in range(STEPS):
                h.reset()
                t = time.perf_counter()
                step()
                ms.append((time.perf_counter() - t) * 1e3)
            out[name + "_step_ms_median"] = statistics.median(ms)
            out[name + "_step_ms_min"] = min(ms)
        if geo:
            kms, launches = h.dns_geo_timing(reset=True)
            out["kernel_ms"] = {k: v / max(launches, 1) for k, v in kms.items()}
            out["kernel_launches"] = launches
        d = h.window_json()["dns"]
        out["query_ecs"] = d["wire_packets"]["query_ecs"]
        out["filtered"] = d["wire_packets"]["filtered"]
        out["top_asn_ecs_head"] = d["top_asn_ecs"][:3]
        return out
    finally:
        h.close()


def main():
    blob, distinct = capture(N)
    buf = np.frombuffer(blob + bytes(4096), dtype=np.uint8).copy()
    idx = pa.RecordIndex(buf[:len(blob)], max_records=N)
    d_recs = torch.from_numpy(buf).cuda()
    d_offs = torch.from_numpy(idx.offsets).cuda()
    torch.cuda.synchronize()
    res = {"queries": N, "distinct_subnets": distinct, "steps": STEPS, "bytes": len(blob)}
    for name, geo, filt in (("no_database", False, False), ("counts", True, False), ("counts_and_filters", True, True),
                            ("no_database_again", False, False), ("counts_again", True, False),
                            ("counts_and_filters_again", True, True)):
        res[name] = phase(d_recs, d_offs, idx, geo, filt)
        print(name, json.dumps(res[name]), flush=True)
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
