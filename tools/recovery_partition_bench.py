#!/usr/bin/env python3
"""Time ramcrc_recovery_partition_device beside the walk before it, the append
after it and a device-to-device copy of the same bytes.

    python tools/recovery_partition_bench.py [--nseg 512] [--values 64,1024,4096]
                                             [--out profiles/recovery_partition]

Sources are RecoverSegmentBenchmark-shaped 8 MiB segments built on the device
(fill_objects: table 0, 8-byte counter keys).  build needs a SEGHEADER before
the first record it places, so the first entry of every segment is retyped to
one (its payload bytes 8..15, the segment id, are zero) and the segments are
certified again.  64 tablets split table 0's hash space evenly over 8
partitions, so every object is placed once.

In one run the four calls alternate -- partition, walk, append (of the list the
partition wrote), copy (torch's copy_ of uint8 tensors, which issues
hipMemcpyAsync, over as many bytes as the segments hold) -- each bracketed by
device events; the medians are over --calls calls after --warmup warm-up
rounds.  One JSON file per value size, and one summary line on stdout.

Each value size is measured in a child process of its own under a time limit;
this process never opens the GPU.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20


def measure(args, value_len):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("recovery_partition_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg, n_part, n_tab = 8 * MiB, args.nseg, 8, 64
    out_stride = cap // n_part + cap // n_part // 4   # room for an uneven split
    n_out = nseg * n_part
    d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    d.random_(0, 256)
    dc = torch.zeros((nseg, 2), dtype=torch.int32, device="cuda")
    per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, value_len, certs=dc)
    first = d.view(nseg, cap)[:, 0]
    first.copy_((first & 0xC0) | segments.LOG_ENTRY_TYPE_SEGHEADER)
    heads = torch.full((nseg,), seg_len, dtype=torch.int32, device="cuda")
    ctx.certify(d, cap, cap, nseg, heads, dc)
    ecap = nseg * (per + 1)
    status = torch.zeros((nseg, 4), dtype=torch.int32, device="cuda")
    entries = torch.zeros((ecap, 4), dtype=torch.int32, device="cuda")
    n_entries = torch.zeros(1, dtype=torch.int64, device="cuda")
    step = (1 << 64) // n_tab
    tabs = segments.tablets_tensor(
        [(0, i * step, (1 << 64) - 1 if i == n_tab - 1 else (i + 1) * step - 1, 0, 0, i % n_part)
         for i in range(n_tab)])
    place = torch.zeros((ecap, 2), dtype=torch.int32, device="cuda")
    n_place = torch.zeros(1, dtype=torch.int64, device="cuda")
    key_hash = torch.zeros(ecap, dtype=torch.int64, device="cuda")
    pstat = torch.zeros((nseg, 4), dtype=torch.int32, device="cuda")
    out = torch.empty(n_out * out_stride, dtype=torch.uint8, device="cuda")
    o_certs = torch.zeros((n_out, 2), dtype=torch.int32, device="cuda")
    o_stat = torch.zeros((n_out, 2), dtype=torch.int32, device="cuda")

    def walk():
        ctx.segment_walk(d, cap, cap, nseg, dc, status, entries, n_entries)

    def partition():
        ctx.recovery_partition(d, cap, nseg, status, entries, n_entries, tabs, n_part, place,
                               n_place, pstat, key_hash=key_hash, n_tablets=n_tab)

    def append():
        ctx.recovery_append(d, cap, nseg, status, entries, n_entries, place, n_place, n_part, out,
                            out_stride, out_stride, o_certs, o_stat)

    src, dst = d[:nseg * seg_len], out[:nseg * seg_len]
    calls = {"partition": partition, "walk": walk, "append": append, "memcpy": lambda: dst.copy_(src)}
    for _ in range(args.warmup):
        walk()
        partition()
        append()
        dst.copy_(src)
    ctx.check()
    n, placed = int(n_entries.item()), int(n_place.item())
    ps = pstat.cpu().numpy().view(np.uint32)
    ost = o_stat.cpu().numpy().view(np.uint32)
    assert n == nseg * per and placed == n - nseg, (n, placed)
    assert (ps[:, 0] == segments.SEG_OK).all() and int(ps[:, 1].sum()) == placed and not ps[:, 2:].any()
    assert (ost[:, 0] == segments.SEG_OK).all() and int(ost[:, 1].sum()) == placed
    per_part = np.bincount(place[:placed, 1].cpu().numpy(), minlength=n_part)

    ms = {k: [] for k in calls}
    for _ in range(args.calls):   # alternate, so that none has the quieter part of the run
        for k, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    ctx.check()
    tiles = (n + 1023) // 1024
    # 16 B per record twice (k_part_heads, k_part_classify), one or two 128-byte
    # lines for the table id and the key, the 8-byte count written once and read
    # twice, the tile sums, 8 B per hash and per placement written
    entry = segments.entry_bytes(value_len)
    record_lines = min(128, entry) * n
    traffic = 2 * 16 * n + record_lines + 3 * 8 * n + 3 * 8 * tiles + 8 * n + 8 * placed
    med = {k: float(np.median(v)) for k, v in ms.items()}
    r = {"value_len": value_len, "nseg": nseg, "segment_bytes": cap, "n_part": n_part,
         "tablets": n_tab, "records": n, "placements": placed, "segment_bytes_used": nseg * seg_len,
         "placements_per_partition": per_part.tolist(),
         "algorithmic_traffic_bytes": {"records_16B_two_passes": 2 * 16 * n,
                                       "record_lines": record_lines, "counts_scratch": 3 * 8 * n,
                                       "scan_words": 3 * 8 * tiles, "hashes": 8 * n,
                                       "placements": 8 * placed, "total": traffic},
         "partition_GBps_of_traffic": traffic / med["partition"] / 1e6,
         "calls_timed": args.calls, "warmup": args.warmup,
         "device": torch.cuda.get_device_name(0), "build": ramcrc.lib().ramcrc_build_info().decode()}
    r["ms_median_min_max"] = {k: [round(med[k], 4), round(min(v), 4), round(max(v), 4)]
                              for k, v in ms.items()}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"partition_{nseg}x8MiB_v{value_len}.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                + "\n}\n")   # one key per line
    ctx.close()
    print(json.dumps({"recovery_partition": dict(value_len=value_len, records=n,
                                                 **{k + "_ms_median": med[k] for k in ms})}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--values", type=lambda s: [int(v) for v in s.split(",")], default=[64, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=15, help="timed calls of each kind, alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recovery_partition"))
    ap.add_argument("--time-limit", type=int, default=180, help="seconds per value size")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        measure(args, args.child)
        return 0
    for value_len in args.values:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(value_len)] + sys.argv[1:]
        try:
            rc = subprocess.run(cmd, timeout=args.time_limit).returncode
        except subprocess.TimeoutExpired:
            print("recovery_partition_bench: a GPU step exceeded its time limit", file=sys.stderr)
            return 124
        if rc:
            return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
