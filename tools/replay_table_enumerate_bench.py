#!/usr/bin/env python3
"""Time a whole-table enumeration from the replay table
(ramcrc_replay_table_enumerate_device) beside the multi-read of the same keys
by key, beside ramcrc_replay_table_stats_device (one pass over the slots), and
beside a device-to-device copy of exactly the payload's bytes.

    python tools/replay_table_enumerate_bench.py [--nseg 512] [--batches 8]
                                                 [--values 64,1024,4096]
                                                 [--out profiles/replay_table_enumerate]

The table is replay_table_read_hashes_bench.py's: RecoverSegmentBenchmark-shaped
8 MiB segments built on the device (fill_objects: table 0, 8-byte counter
keys), the first entry of every segment retyped to a SEGHEADER, walked as
--batches batches and added batch by batch with the partition call's hashes.

One round enumerates the whole table (table 0, every hash, no stale frame, no
bucket limit) into one payload buffer just under 4 GiB, from cursor (0, 0) in
as many calls as the cursor needs: a call's summary is read on the host for the
next call's cursor, and every call writes from the buffer's start.  The round
does this with full objects and with keys only, then the multi-read of the same
keys (default mode, hashes given, no rules, d_part_off and d_results NULL), the
stats call, and a copy of each call's payload_bytes (torch's copy_ of uint8
tensors, which issues hipMemcpyAsync).  Each is bracketed by device events; an
enumeration's time is the sum over its calls.  The per-kernel split comes from
a call that can send nothing (max_bytes 0: k_en_size and k_en_scan run whole,
k_en_gather finds no tile): its time is the two passes', and the rest of a
first call's time is the gather's.  Medians are over --calls rounds after
--warmup warm-up rounds.  Every call's summary is checked, the totals against
the table's keys, and the first entries of a payload against their lengths.

One JSON file per value size, and one summary line each on stdout.  Each value
size is measured in a child process of its own under a time limit; this process
never opens the GPU.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
MAXH = (1 << 64) - 1


def measure(args, value_len):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments
    from replay_table_bench import Walk

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_table_enumerate_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg, nb = 8 * MiB, args.nseg, args.batches
    assert nseg % nb == 0
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")

    d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    d.random_(0, 256)
    dc = z((nseg, 2), torch.int32)
    per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, value_len, first_key=0, certs=dc)
    first = d.view(nseg, cap)[:, 0]
    first.copy_((first & 0xC0) | segments.LOG_ENTRY_TYPE_SEGHEADER)
    ctx.certify(d, cap, cap, nseg, torch.full((nseg,), seg_len, dtype=torch.int32, device="cuda"), dc)
    parts = [Walk(torch, ctx, segments, d, dc, cap, b * (nseg // nb), nseg // nb, per) for b in range(nb)]
    for p in parts:
        p.walk(ctx)
    keys, hashes = [], []
    for p in parts:
        ne = int(p.n_entries.item())
        e = p.entries[:ne].long()
        rec = torch.nonzero((e[:, 3] & 0x3F) == segments.LOG_ENTRY_TYPE_OBJ).reshape(-1)
        e = e[rec]
        at = e[:, 0] * cap + e[:, 1] + 1 + ((e[:, 3] >> 6) & 3) + 1 + 27
        keys.append(p.d[at[:, None] + torch.arange(8, device="cuda")])
        hashes.append(p.key_hash[rec])
    keybuf, hashes = torch.cat(keys).contiguous().reshape(-1), torch.cat(hashes).contiguous()
    del keys
    n = hashes.shape[0]
    assert n == nseg * (per - 1), (n, nseg, per)
    queries = z((n, 3), torch.int64)   # table 0, key_off, key_len 8 (reserved 0)
    queries[:, 1] = 8 * torch.arange(n, device="cuda")
    queries[:, 2] = 8
    kv = 1 + 2 + 8 + value_len   # key count, one cumulative length, the key, the value
    entry = {False: 4 + 24 + kv, True: 4 + 24 + 11}
    room = (4 << 30) - 4096   # just under 4 GiB
    payload = torch.empty(room, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty(room, dtype=torch.uint8, device="cuda")
    reply = payload if n * (16 + kv) <= room else torch.empty(n * (16 + kv), dtype=torch.uint8, device="cuda")
    en_summary, rd_summary, stats = z(11, torch.int64), z(10, torch.int64), z(6, torch.int64)
    table = ramcrc.ReplayTable(ctx, nseg * per, nb)
    for p in parts:
        table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work, key_hash=p.key_hash)
    ctx.check()

    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def got(summary, dt):
        s = summary.cpu().numpy().view(dt)[0]
        return {k: int(s[k]) for k in dt.names}

    def enumerate_all(keys_only, check_entries=False):
        """(ms, calls, per-call payload bytes) of the whole table from (0, 0)."""
        bucket = nxt = 0
        ms, sizes, objects, slots = 0.0, [], 0, None
        while slots is None or bucket < slots:
            ms += timed(lambda: table.enumerate(0, payload, en_summary, room, bucket_index=bucket,
                                                bucket_next_hash=nxt, keys_only=keys_only))
            s = got(en_summary, segments.ENUMERATE_SUMMARY_DTYPE)
            assert s["spoiled"] == 0 and s["stuck"] == 0 and s["tombstones"] == 0, s
            assert s["payload_bytes"] == s["objects"] * entry[keys_only] <= room, s
            assert (s["next_bucket"], s["next_hash"]) > (bucket, nxt), s
            if check_entries and s["objects"]:
                head = payload[:8 * entry[keys_only]].cpu().numpy()
                for k in range(8):
                    e = head[k * entry[keys_only]:(k + 1) * entry[keys_only]]
                    assert int(e[:4].view("<u4")[0]) == entry[keys_only] - 4 and e[4 + 24] == 1 and e[4 + 25] == 8, k
            slots = s["num_buckets"]
            sizes.append(s["payload_bytes"])
            objects += s["objects"]
            bucket, nxt = s["next_bucket"], s["next_hash"]
        assert objects == n, (objects, n)
        return ms, len(sizes), sizes

    def nothing_sent():
        """k_en_size and k_en_scan alone: a call with no room sends nothing."""
        t = timed(lambda: table.enumerate(0, payload, en_summary, 0, payload_capacity=room))
        s = got(en_summary, segments.ENUMERATE_SUMMARY_DTYPE)
        assert s["objects"] == 0 and s["full"] == 1 and s["payload_bytes"] == 0, s
        return t

    def first_call(keys_only):
        return timed(lambda: table.enumerate(0, payload, en_summary, room, keys_only=keys_only))

    def one_round():
        t_full, calls_full, sizes = enumerate_all(False)
        t_keys, calls_keys, _ = enumerate_all(True)
        t_first = first_call(False)
        t_passes = nothing_sent()
        t_read = timed(lambda: table.read(keybuf, queries, reply, rd_summary, key_hash=hashes))
        s = got(rd_summary, segments.READ_SUMMARY_DTYPE)
        assert s["returned"] == n and s["ok"] == n and s["reply_bytes"] == n * (16 + kv), s
        t_stats = timed(lambda: table.stats(stats))
        st = got(stats, segments.REPLAY_TABLE_STATS_DTYPE)
        assert st["keys"] == n and st["live_objects"] == n, st
        t_copy = sum(timed(lambda: copy_dst[:b].copy_(payload[:b])) for b in sizes)
        return dict(enumerate=t_full, enumerate_keys_only=t_keys, first_call=t_first, size_and_scan=t_passes,
                    gather_of_first_call=t_first - t_passes, read=t_read, stats=t_stats, copy=t_copy), \
            calls_full, calls_keys, sizes

    for _ in range(args.warmup):
        one_round()
    ctx.check()
    enumerate_all(False, check_entries=True)
    enumerate_all(True, check_entries=True)
    ms, calls_full, calls_keys, sizes = {}, 0, 0, []
    for _ in range(args.calls):
        r, calls_full, calls_keys, sizes = one_round()
        for k, v in r.items():
            ms.setdefault(k, []).append(v)
    ctx.check()
    mmm = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
    ratio = lambda a, b: mmm([x / y for x, y in zip(ms[a], ms[b])])
    total = sum(sizes)
    r = {"value_len": value_len, "nseg": nseg, "batches": nb, "segment_bytes": cap, "keys": n,
         "slots": got(en_summary, segments.ENUMERATE_SUMMARY_DTYPE)["num_buckets"],
         "payload_capacity": room, "payload_bytes": total, "payload_bytes_keys_only": n * entry[True],
         "calls_full": calls_full, "calls_keys_only": calls_keys, "calls_timed": args.calls, "warmup": args.warmup,
         "device": torch.cuda.get_device_name(0), "build": ramcrc.lib().ramcrc_build_info().decode(),
         "ms_median_min_max": {k: mmm(v) for k, v in ms.items()},
         "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
         "enumerate_GBps_of_payload": round(total / 1e6 / float(np.median(ms["enumerate"])), 2),
         "ratio_enumerate_over_read_median_min_max": ratio("enumerate", "read"),
         "ratio_enumerate_over_stats_median_min_max": ratio("enumerate", "stats"),
         "ratio_enumerate_over_copy_median_min_max": ratio("enumerate", "copy"),
         "ratio_keys_only_over_stats_median_min_max": ratio("enumerate_keys_only", "stats"),
         "share_size_and_scan_of_first_call_median_min_max": ratio("size_and_scan", "first_call")}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"enumerate_{nseg}x8MiB_b{nb}_v{value_len}.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                + "\n}\n")   # one key per line
    print(json.dumps({"replay_table_enumerate": dict(
        value_len=value_len, keys=n, slots=r["slots"], payload_bytes=total, calls_full=calls_full,
        calls_keys_only=calls_keys, GBps=r["enumerate_GBps_of_payload"],
        over_read=r["ratio_enumerate_over_read_median_min_max"],
        over_stats=r["ratio_enumerate_over_stats_median_min_max"],
        over_copy=r["ratio_enumerate_over_copy_median_min_max"],
        **{k + "_ms": v for k, v in r["ms_median_min_max"].items()})}), flush=True)
    table.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--values", type=lambda s: [int(v) for v in s.split(",")], default=[64, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=7, help="timed rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_table_enumerate"))
    ap.add_argument("--time-limit", type=int, default=240, help="seconds per value size")
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
            print("replay_table_enumerate_bench: a GPU step exceeded its time limit", file=sys.stderr)
            return 124
        if rc:
            return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
