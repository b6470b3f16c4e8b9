#!/usr/bin/env python3
"""Drive the GeoIP device walker (pv_geo_walk) over the IPv4 addresses of a synthetic batch, for a
kernel-trace run:

    rocprofv3 --kernel-trace --stats --output-format csv -d out -o k -- \\
        python tools/geo_walk_time.py --asn big.mmdb --config 2 --records 1000000

With `--pipeline` the batch itself goes through pv_process_host `--reps` times with the databases
attached, so the trace holds pv_geo_count (one walk per combined IP entry) next to the passes
it rides behind. Otherwise each attached database is walked `--reps` times over (a) one address
per record (its source when that is outside the host subnet, else its destination: the address
the Net handler counts) and
(b) the distinct addresses among them (what the top-N combine lists hold). The kernel times are
the profiler's; this script prints the address counts, the share of "Unknown" and a wall-clock
figure that includes the copies."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def batch_addresses(cfg: int, n: int) -> np.ndarray:
    """(n, 4) uint8: the remote IPv4 address of every Ethernet/IPv4 record of a synthetic batch"""
    from pktvisor_amd import synth
    buf, offs, _ = synth.records(cfg, n, with_offsets=True)
    offs = offs.astype(np.int64)
    eth = (buf[offs + 16 + 12].astype(np.uint16) << 8) | buf[offs + 16 + 13]
    offs = offs[eth == 0x0800]
    src = np.stack([buf[offs + 16 + 14 + 12 + k] for k in range(4)], axis=1)
    dst = np.stack([buf[offs + 16 + 14 + 16 + k] for k in range(4)], axis=1)
    host = int(synth.HOST_SPEC.split(".")[0])  # 10.0.0.0/8
    return np.ascontiguousarray(np.where((src[:, :1] == host), dst, src))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--city")
    ap.add_argument("--asn")
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pipeline", action="store_true", help="time pv_geo_count inside pv_process_host instead")
    a = ap.parse_args()
    import torch  # (its HIP runtime first, as bench.py does)
    torch.cuda.init()
    import pktvisor_amd as pa
    if a.pipeline:
        from pktvisor_amd import synth
        buf, _, used = synth.records(a.config, a.records)
        h = pa.PvHandlers(host_spec=synth.HOST_SPEC, num_periods=1, max_records=a.records, geo_city_db=a.city, geo_asn_db=a.asn)
        h.process_host(buf[:used])  # warm-up
        t0 = time.perf_counter()
        for _ in range(a.reps):
            h.process_host(buf[:used])
        dt = (time.perf_counter() - t0) / a.reps
        p = h.window_json(0)["packets"]
        print(f"pipeline: {a.records} records of config {a.config}, {dt * 1e3:.3f} ms per pv_process_host call; "
              f"top_geoLoc {p['top_geoLoc'][:2]} top_ASN {p['top_ASN'][:2]}")
        h.close()
        return
    per_record = batch_addresses(a.config, a.records)
    distinct = np.unique(per_record.view(np.uint32).reshape(-1)).view(np.uint8).reshape(-1, 4)
    rng = np.random.default_rng(1)
    uniform = rng.integers(0, 256, size=per_record.shape, dtype=np.uint8)
    h = pa.PvHandlers(host_spec="10.0.0.0/8", num_periods=1, max_records=1 << 12)
    dbs = {k: pa.GeoDB(p, k) for k, p in (("city", a.city), ("asn", a.asn)) if p}
    h.set_geodb(dbs.get("city"), dbs.get("asn"))
    for kind, db in dbs.items():
        for label, addrs in (("per_record", per_record), ("distinct", distinct), ("uniform_random", uniform)):
            ids = h.geo_lookup_device(kind, addrs, 4)  # warm-up, and the check against the host walk
            assert np.array_equal(ids, db.lookup_ids(addrs, 4))
            t0 = time.perf_counter()
            for _ in range(a.reps):
                h.geo_lookup_device(kind, addrs, 4)
            dt = (time.perf_counter() - t0) / a.reps
            print(f"{kind} {label}: {len(addrs)} addresses, {len(db.entries)} dictionary entries, "
                  f"unknown {float((ids == 0).mean()):.3f}, {dt * 1e3:.3f} ms per call with copies")
    h.close()


if __name__ == "__main__":
    main()
