"""Cost of the attached flow stage: pv_flow_scan next to pv_dhcp_scan on the 10M-record C2 blob
(no datagram found), and on a synthetic batch of NetFlow v5 datagrams with 30 records each."""
import json
import os
import struct
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pktvisor_amd as pa  # noqa: E402
from pktvisor_amd import synth  # noqa: E402
from tests import flow_cases as fc  # noqa: E402

out = {}
dev = torch.device("cuda:0")
WARM, STEPS = 3, 10


def run(h, d_recs, d_offs, idx, warm=WARM, steps=STEPS):
    for _ in range(warm):
        h.reset()
        h.process_device(d_recs.data_ptr(), d_offs.data_ptr(), idx)
        h.synchronize()
    h.reset()
    h.set_kernel_timing(1)
    for t in (h.dhcp_timing, h.flow_timing):
        t(reset=True)
    h.kernel_timing(reset=True)
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        h.process_device(d_recs.data_ptr(), d_offs.data_ptr(), idx)
        h.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    d, dn = h.dhcp_timing()
    f, fn = h.flow_timing()
    k, kn = h.kernel_timing()
    return {"step_ms_median": float(np.median(ms)), "step_ms_min": float(min(ms)), "dhcp_scan_ms": d / max(dn, 1), "dhcp_launches": dn,
            "flow_scan_ms": f / max(fn, 1), "flow_launches": fn, "net_pass_ms": k / max(kn, 1), "flow_stats": h.flow_stats()}


# ---- C2
n = 10_000_000
buf, offs, used = synth.records(2, n, seed=synth.SEEDS[2], with_offsets=False)
idx = pa.RecordIndex(buf[:used], max_records=n)
d_recs = torch.from_numpy(buf).to(dev)
d_offs = torch.from_numpy(idx.offsets).to(dev)
for name, ports in (("c2_port_2055", [2055]), ("c2_any_udp", [])):
    h = pa.PvHandlers(host_spec=synth.HOST_SPEC, num_periods=5, max_records=n, dhcp_config={},
                      flow_config={"ports": ports, "disable": ["all"]}, deep_sample_rate=1)
    out[name] = run(h, d_recs, d_offs, idx)
    h.close()
    print(name, json.dumps(out[name]), flush=True)
del d_recs, d_offs

# ---- every record a v5 datagram with 30 flow records
nd = 100_000
one = np.frombuffer(fc.packet(fc.datagram(5, fc.flows_n(30)), fc.T0), dtype=np.uint8)
blob = np.zeros(len(one) * nd + 256, dtype=np.uint8)
blob[:len(one) * nd] = np.tile(one, nd)
idx = pa.RecordIndex(blob[:len(one) * nd], max_records=nd)
assert idx.n == nd
d_recs = torch.from_numpy(blob).to(dev)
d_offs = torch.from_numpy(idx.offsets).to(dev)
h = pa.PvHandlers(host_spec=synth.HOST_SPEC, num_periods=5, max_records=nd, dhcp_config={},
                  flow_config={"ports": [2055], "disable": ["all"]}, deep_sample_rate=1)
out["v5_30_records"] = dict(run(h, d_recs, d_offs, idx, warm=1, steps=3), datagrams=nd, record_bytes=int(len(one)))
h.close()
print("v5", json.dumps(out["v5_30_records"]), flush=True)
os.makedirs(os.path.join(ROOT, "profiles", "flow"), exist_ok=True)
json.dump(out, open(os.path.join(ROOT, "profiles", "flow", "c2_measure.json"), "w"), indent=1)
