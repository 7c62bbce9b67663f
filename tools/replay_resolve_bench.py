#!/usr/bin/env python3
"""Time ramcrc_replay_resolve_device beside the walk and the partition call
before it and a device-to-device copy of the same bytes.

    python tools/replay_resolve_bench.py [--nseg 512] [--values 64,1024,4096]
                                         [--out profiles/replay_resolve]

Sources are RecoverSegmentBenchmark-shaped 8 MiB segments built on the device
(fill_objects: table 0, 8-byte counter keys, version 0), the first entry of
every segment retyped to a SEGHEADER as in recovery_partition_bench.py so that
the partition call, which supplies the hashes, places the rest.  Two shapes per
value size: `distinct` (every key once) and `twice` (the second half of the
segments are byte copies of the first half, so every key occurs twice and the
record earlier in the walk's table wins).

In one run the five calls alternate -- resolve with the partition call's
hashes, resolve with NULL hashes, walk, partition, copy (torch's copy_ of uint8
tensors, which issues hipMemcpyAsync, over as many bytes as the segments hold)
-- each bracketed by device events; the medians are over --calls calls after
--warmup warm-up rounds.  One JSON file per value size and shape, and one
summary line each on stdout.

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


def slots_for(n):
    s = 64
    while s < 2 * n:
        s *= 2
    return s


def measure(args, value_len):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_resolve_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg = 8 * MiB, args.nseg
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
    tabs = segments.tablets_tensor([(0, 0, (1 << 64) - 1, 0, 0, 0)])
    place = torch.zeros((ecap, 2), dtype=torch.int32, device="cuda")
    n_place = torch.zeros(1, dtype=torch.int64, device="cuda")
    key_hash = torch.zeros(ecap, dtype=torch.int64, device="cuda")
    pstat = torch.zeros((nseg, 4), dtype=torch.int32, device="cuda")
    winner = torch.zeros(ecap, dtype=torch.int32, device="cuda")
    live = torch.zeros((ecap, 2), dtype=torch.int32, device="cuda")
    n_live = torch.zeros(1, dtype=torch.int64, device="cuda")
    counts = torch.zeros(6, dtype=torch.int64, device="cuda")
    copy_dst = torch.empty(nseg * seg_len, dtype=torch.uint8, device="cuda")
    ctx.reserve(16 + 6 * slots_for(ecap), 2 * ecap)

    def walk():
        ctx.segment_walk(d, cap, cap, nseg, dc, status, entries, n_entries)

    def partition():
        ctx.recovery_partition(d, cap, nseg, status, entries, n_entries, tabs, 1, place, n_place,
                               pstat, key_hash=key_hash, n_tablets=1)

    def resolve(hashes):
        ctx.replay_resolve(d, cap, nseg, status, entries, n_entries, live, n_live, counts,
                           key_hash=hashes, winner=winner)

    src = d[:nseg * seg_len]
    calls = {"resolve_given": lambda: resolve(key_hash), "resolve_null": lambda: resolve(None),
             "walk": walk, "partition": partition, "memcpy": lambda: copy_dst.copy_(src)}
    for shape in ("distinct", "twice"):
        if shape == "twice":
            half = nseg // 2
            d.view(nseg, cap)[half:2 * half].copy_(d.view(nseg, cap)[:half])
            dc[half:2 * half].copy_(dc[:half])
        for _ in range(args.warmup):
            walk()
            partition()
            resolve(key_hash)
            resolve(None)
            copy_dst.copy_(src)
        ctx.check()
        n, kept = int(n_entries.item()), int(n_live.item())
        ct = counts.cpu().numpy().view(segments.RESOLVE_COUNTS_DTYPE)[0]
        keys = n - nseg if shape == "distinct" else (n - nseg) - (nseg // 2) * (per - 1)
        assert n == nseg * per and int(ct["objects"]) == n - nseg, (n, ct)
        assert kept == keys == int(ct["live_objects"]), (shape, kept, keys, ct)
        if shape == "twice":   # a record and its twin share the winner, one of the two
            seg, off = entries[:n, 0].long(), entries[:n, 1]
            w = winner[:n].long()
            p = w >= 0
            ws = seg[w[p]]
            assert bool((entries[w[p], 1] == off[p]).all())
            assert bool(((ws == seg[p]) | (ws == seg[p] - nseg // 2) | (ws == seg[p] + nseg // 2)).all())

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
        assert int(n_live.item()) == kept
        tiles, slots = (n + 1023) // 1024, slots_for(n)
        parts = n - nseg
        entry = segments.entry_bytes(value_len)
        # what the algorithm has to move, with the hashes given:
        #   records     16 B per record in k_res_insert, k_res_pick and k_res_tiles
        #   hashes      8 B per record (its own; a claimant's only on a collision)
        #   key lines   the line(s) of a record's header and key, min(128, entry)
        #               bytes; a record that finds its key claimed reads the
        #               claimant's as well
        #   slots       24 B per slot zeroed; per participant a 4-byte claim
        #               read or CAS, an 8-byte version max and read, an 8-byte
        #               pick max and read
        #   scratch     version and slot per record written and read (8 B each),
        #               the winner written back and read by k_res_emit
        #   outputs     4 B per winner slot, 8 B per live record, the tile sums
        t = {"records_16B_three_passes": 3 * 16 * n, "hashes": 8 * parts,
             "key_lines": min(128, entry) * (parts + (parts - kept)),
             "slots_zeroed": 24 * slots, "slot_words_touched": (4 + 16 + 16) * parts,
             "record_scratch": (16 + 16 + 16) * n, "winner": 4 * n, "live": 8 * kept,
             "scan_words": 3 * 8 * tiles}
        t["total"] = sum(t.values())
        med = {k: float(np.median(v)) for k, v in ms.items()}
        r = {"shape": shape, "value_len": value_len, "nseg": nseg, "segment_bytes": cap, "records": n,
             "participants": parts, "live": kept, "table_slots": slots,
             "segment_bytes_used": nseg * seg_len, "algorithmic_traffic_bytes": t,
             "resolve_given_GBps_of_traffic": t["total"] / med["resolve_given"] / 1e6,
             "resolve_given_records_per_us": n / med["resolve_given"] / 1e3,
             "calls_timed": args.calls, "warmup": args.warmup,
             "device": torch.cuda.get_device_name(0), "build": ramcrc.lib().ramcrc_build_info().decode()}
        r["ms_median_min_max"] = {k: [round(med[k], 4), round(min(v), 4), round(max(v), 4)]
                                  for k, v in ms.items()}
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"resolve_{nseg}x8MiB_v{value_len}_{shape}.json"), "w") as f:
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                    + "\n}\n")   # one key per line
        print(json.dumps({"replay_resolve": dict(shape=shape, value_len=value_len, records=n, live=kept,
                                                 **{k + "_ms": r["ms_median_min_max"][k] for k in ms})}),
              flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--values", type=lambda s: [int(v) for v in s.split(",")], default=[64, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=15, help="timed calls of each kind, alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_resolve"))
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
            print("replay_resolve_bench: a GPU step exceeded its time limit", file=sys.stderr)
            return 124
        if rc:
            return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
