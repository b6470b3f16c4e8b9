"""The cost of the v2 handlers' geo half (pv_set_v2_geo) on a device-resident C4-shaped batch
(pktvisor_amd.synth config 4: IMIX plus DNS query / response pairs) with Net v1, Net v2 and DNS v2
(top_ecs enabled) attached: the step time with the databases detached, with both test databases
counted (v1's top_geoLoc / top_ASN and Net v2's per-direction tops in one pv_geo_count launch, DNS
v2's by pv_dns2_ecs_geo), and with both v2 handlers' geoloc_notfound / asn_notfound filters on top;
and, by HIP events through the kernel-timing switch (pv_v2_geo_timing, pv_dns_geo_timing),
pv_geo_count, the v2 pv_geo_verdict launch, pv_dns2_ecs_geo and pv_dns_geo_verdict of the same runs
(DESIGN; profiles/geo_v2/measure.json).
Usage: python tools/geo_v2_measure.py [RECORDS [OUT.json]]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pktvisor_amd as pa  # noqa: E402
from pktvisor_amd import synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else None
STEPS, WARMUP = 10, 2
GOLD = os.path.join(ROOT, "tests", "golden")
CITY, ISP = os.path.join(GOLD, "GeoIP2-City-Test.mmdb"), os.path.join(GOLD, "GeoIP2-ISP-Test.mmdb")


def phase(d_recs, d_offs, idx, geo: bool, filters: bool):
    kw = dict(geo_city_db=CITY, geo_asn_db=ISP, v2_geo=True) if geo else {}
    n2 = {"geoloc_notfound": True, "asn_notfound": True} if filters else {}
    d2 = {"enable": ["top_ecs"], **n2}
    h = pa.PvHandlers(host_spec=synth.HOST_SPEC, num_periods=5, max_records=N, device=0, net_config={},
                      net2_config=n2, dns2_config=d2, **kw)
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
                h.v2_geo_timing(reset=True)
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
            kms, launches = h.v2_geo_timing(reset=True)
            out["kernel_ms"] = {k: v / max(launches, 1) for k, v in kms.items()}
            out["kernel_launches"] = launches
            dms, dl = h.dns_geo_timing(reset=True)  # (stamped only while the DNS v2 geo filters are on)
            out["kernel_ms"]["pv_dns_geo_verdict"] = dms["pv_dns_geo_verdict"] / dl if dl else None
        win = h.window_json()
        net = win["net"]
        out["dns_filtered_packets"] = win["dns"]["filtered_packets"]
        out["dns_ecs_xacts"] = {d: win["dns"][d].get("ecs_xacts") for d in ("in", "out", "unknown") if d in win["dns"]}
        out["observed_packets"] = net["observed_packets"]
        out["filtered_packets"] = net["filtered_packets"]
        out["top_asn_packets_head"] = {d: net[d]["top_asn_packets"][:2] for d in ("in", "out", "unknown") if d in net}
        return out
    finally:
        h.close()


def main():
    blob = synth.pcap_bytes(4, N)[24:]
    buf = np.frombuffer(blob + bytes(4096), dtype=np.uint8).copy()
    idx = pa.RecordIndex(buf[:len(blob)], max_records=N)
    d_recs = torch.from_numpy(buf).cuda()
    d_offs = torch.from_numpy(idx.offsets).cuda()
    torch.cuda.synchronize()
    res = {"records": N, "steps": STEPS, "bytes": len(blob)}
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
