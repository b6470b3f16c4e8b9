"""Rank process of the sharded Net v2 geo test (tests/test_gpu_geo2.py), in the pattern of
tests/geo_dist_worker.py: rank r processes the contiguous shard r of a pcap with the GeoIP
databases attached and the v2 geo switch on (Net v1, Net v2 and DNS v2), the ranks merge with
pktvisor_amd.dist.merge_window, rank 0 writes the window JSON.

usage: python -m tests.geo2_dist_worker PCAP OUT HOST_SPEC CITY_DB ASN_DB [ASN_DB_OF_THE_OTHER_RANKS]"""
import json
import os
import struct
import sys


def main(pcap_path, out, host, city, asn, asn_other=None):
    import torch
    import torch.distributed as dist
    import pktvisor_amd as pa
    from pktvisor_amd import dist as pvdist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    torch.cuda.init()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    linktype, ts_nano, recs = pa.read_pcap(pcap_path)
    idx = pa.RecordIndex(recs, ts_nano)
    cuts = pa.shard_cuts(recs, idx, linktype, ts_nano, world)
    lo, hi = cuts[rank], cuts[rank + 1]
    offs = [int(x) for x in idx.offsets] + [len(recs)]
    h = pa.PvHandlers(host_spec=host, num_periods=1, topn_count=50, linktype=linktype, ts_nano=ts_nano,
                      max_records=max(1, hi - lo), device=dev.index, geo_city_db=city,
                      geo_asn_db=asn_other if (asn_other and rank) else asn, net2_config={}, dns2_config={"enable": ["top_ecs"]}, v2_geo=True)
    try:
        h.set_global_base(lo)
        sec, frac = struct.unpack_from("<II", recs, offs[0])
        shard = recs[offs[lo]:offs[hi]]
        pvdist.process_shard(h, shard, pa.RecordIndex(shard, ts_nano) if hi > lo else None, sec, frac * 1000)
        h.set_end_tstamp(*pa.last_record_ts(recs, idx, ts_nano))
        pvdist.merge_window(h, dev)
        if rank == 0:
            json.dump({"1m": h.window_json(0)}, open(out, "w"))
    finally:
        h.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main(*sys.argv[1:])
