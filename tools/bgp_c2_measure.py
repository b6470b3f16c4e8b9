"""C2 (bench.py's flagship workload, device resident) with and without the BGP handler attached:
step time, the Net pass's device time and pv_bgp_scan's from the same run (DESIGN section 9;
profiles/bgp/c2_measure.json). Usage: python tools/bgp_c2_measure.py [RECORDS [OUT.json]]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pktvisor_amd as pa  # noqa: E402
from pktvisor_amd import synth  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else None
STEPS, WARMUP = 20, 3


def phase(d_recs, d_offs, idx, bgp: bool):
    h = pa.PvHandlers(host_spec=synth.HOST_SPEC, num_periods=5, max_records=N, device=0, bgp_config={} if bgp else None)
    try:
        def step():
            h.process_device(d_recs.data_ptr(), d_offs.data_ptr(), idx)
            h.synchronize()
        for _ in range(WARMUP):
            h.reset()
            step()
        h.reset()
        out = {}
        for name, every in (("unstamped", 0), ("stamped", 1)):
            h.set_kernel_timing(every)
            h.kernel_timing(reset=True)
            h.bgp_timing(reset=True)
            ms = []
            for _ in range(STEPS):
                t = time.perf_counter()
                step()
                ms.append((time.perf_counter() - t) * 1e3)
            out[name + "_step_ms_median"] = statistics.median(ms)
            out[name + "_step_ms_min"] = min(ms)
        kms, kl = h.kernel_timing(reset=True)
        bms, bl = h.bgp_timing(reset=True)
        out.update(net_kernel=h.net_kernel_name() if hasattr(h, "net_kernel_name") else None, net_pass_ms=kms / max(kl, 1),
                   net_pass_launches=kl, bgp_scan_ms=bms / max(bl, 1), bgp_scan_launches=bl)
        w = h.window_json()
        out["events"] = w["packets"]["total"] if "total" in w.get("packets", {}) else None
        out["bgp_events"] = w["bgp"]["wire_packets"]["events"] if bgp else None
        return out
    finally:
        h.close()


def main():
    buf, offs, used = synth.records(2, N, seed=synth.SEEDS[2], with_offsets=False)
    idx = pa.RecordIndex(buf[:used], max_records=N)
    d_recs = torch.from_numpy(buf).cuda()
    d_offs = torch.from_numpy(idx.offsets).cuda()
    torch.cuda.synchronize()
    res = {"records": N, "steps": STEPS}
    for name, bgp in (("plain", False), ("bgp", True), ("plain_again", False), ("bgp_again", True)):
        res[name] = phase(d_recs, d_offs, idx, bgp)
        print(name, json.dumps(res[name]), flush=True)
    if OUT:
        with open(OUT, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
