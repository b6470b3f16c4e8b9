"""wrong-guess cost on C2-sized batches: blob A is C2's 10M plain records, blob B the same with one
record's UDP destination port set to 53. Cycles of A A A B B: the first B of a cycle is launched
without the log on a wrong guess (ring kernel, log rebuild, regular chain), the second B runs the
regular chain from the start. The cost of the guess is the difference of the two step times."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import torch
import pktvisor_amd as pa
from pktvisor_amd import synth

n = 10_000_000
buf, offs, used = synth.records(2, n, seed=synth.SEEDS[2], with_offsets=False)
idx = pa.RecordIndex(buf[:used], max_records=n)
bufb = buf.copy()
o = int(idx.offsets[n // 2])
bufb[o + 16 + 14 + 20 + 2:o + 16 + 14 + 20 + 4] = (0, 53)
dev = torch.device("cuda", 0)
da, db = torch.from_numpy(buf).to(dev), torch.from_numpy(bufb).to(dev)
do = torch.from_numpy(idx.offsets).to(dev)
h = pa.PvHandlers(host_spec=synth.HOST_SPEC, num_periods=5, max_records=n, device=0)


def step(d):
    t = time.perf_counter()
    h.process_device(d.data_ptr(), do.data_ptr(), idx)
    h.synchronize()
    return (time.perf_counter() - t) * 1e3


for _ in range(3):
    step(da)
h.reset()
h.ring_stats(reset=True)
h.fuse_stats(reset=True)
h.chain_stats(reset=True)
t = {k: [] for k in "a1 a2 a3 b1 b2".split()}
for c in range(12):
    for k, d in (("a1", da), ("a2", da), ("a3", da), ("b1", db), ("b2", db)):
        t[k].append(step(d))
for k, v in t.items():
    v = np.array(v[2:])
    print(f"{k}: mean {v.mean():.4f} median {np.median(v):.4f} min {v.min():.4f} max {v.max():.4f} ms")
b1, b2 = np.array(t["b1"][2:]), np.array(t["b2"][2:])
print(f"wrong-guess cost (b1 - b2): mean {np.mean(b1 - b2) * 1e3:.1f} us, median {np.median(b1 - b2) * 1e3:.1f} us")
print("ring_stats", h.ring_stats(), "fuse_stats", h.fuse_stats(), "chain_stats", h.chain_stats())
