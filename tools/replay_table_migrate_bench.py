#!/usr/bin/env python3
"""Time a tablet migration out of the replay table
(ramcrc_replay_table_migrate_device) beside three things the library could
already do: a device-to-device copy of exactly the bytes the migration wrote;
the live query of the same batches followed by ramcrc_recovery_append_device at
one partition over the same lists (for the whole hash range in live-only mode,
where both write the same records); and a keys-and-values enumeration of the
same hash range.

    python tools/replay_table_migrate_bench.py [--nseg 512] [--batches 8]
                                               [--values 64,1024,4096]
                                               [--out profiles/replay_table_migrate]

The table is replay_table_clean_bench.py's: RecoverSegmentBenchmark-shaped
8 MiB segments built on the device (fill_objects: table 0, 8-byte counter
keys), the first entry of every segment retyped to a SEGHEADER, walked as
--batches batches and added batch by batch, every object's version set to 1
before the add.  Every key has one record, so both modes send the same records;
live-only mode reads the slots' picks as well.

Three ranges: the whole hash range, its lower half and its lowest tenth; two
modes; 8 MiB transfer segments, as many as the source has.  A migration only
reads the table, so the table is built once.  Every round times, each
bracketed by device events: the migration (d_sent given); the copy of
sent_bytes (torch's copy_ of uint8 tensors, which issues hipMemcpyAsync); the
enumeration of the range, reply after reply until the last bucket, its cursor
read on the host between replies as a master's iterator does; and, for the
whole range in live-only mode, live + append of every batch.  Ratios are taken
round by round, medians over --calls rounds after --warmup warm-up rounds.
Once per case the summary is checked: the whole range sends every object, the
records read are all the batches', and the certificates' heads add up to
sent_bytes.  The transfer segments are not walked here; the tests do that.  One
JSON file per value size, and one summary line each on stdout.

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
M64 = (1 << 64) - 1
RANGES = {"whole": M64, "half": (1 << 63) - 1, "tenth": M64 // 10}   # last_hash; first_hash is 0


def measure(args, value_len):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments
    from replay_table_bench import Walk

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_table_migrate_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg, nb = 8 * MiB, args.nseg, args.batches
    assert nseg % nb == 0
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    d.random_(0, 256)
    dc = z((nseg, 2), torch.int32)
    per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, value_len, first_key=0, certs=dc)
    first = d.view(nseg, cap)[:, 0]
    first.copy_((first & 0xC0) | segments.LOG_ENTRY_TYPE_SEGHEADER)
    ctx.certify(d, cap, cap, nseg, torch.full((nseg,), seg_len, dtype=torch.int32, device="cuda"), dc)
    sb = nseg // nb
    parts = [Walk(torch, ctx, segments, d, dc, cap, b * sb, sb, per) for b in range(nb)]
    n_obj = 0
    for p in parts:
        p.walk(ctx)
        e = p.entries[:int(p.n_entries.item())].long()
        e = e[(e[:, 3] & 0x3F) == segments.LOG_ENTRY_TYPE_OBJ]
        p.d[e[:, 0] * cap + e[:, 1] + 1 + ((e[:, 3] >> 6) & 3) + 1 + 8] = 1   # version 1
        n_obj += e.shape[0]
    n_rec = n_obj + nseg
    lst = list(range(nb))
    max_segs = nseg + 8
    chunks, entries = ramcrc.ReplayTable.migrate_reserve([p.ecap for p in parts], max_segs)
    ctx.reserve(max(chunks, 80 + 4 * sb), max(entries, max(p.ecap for p in parts)))
    table = ramcrc.ReplayTable(ctx, nseg * per + 64, nb + 2)
    for p in parts:
        table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work, key_hash=None)
    ctx.check()

    out = torch.empty(max_segs * cap, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty(max_segs * cap, dtype=torch.uint8, device="cuda")
    certs, counts = z((max_segs, 2), torch.int32), z((max_segs, 4), torch.int32)
    sent, seg_first, summary = z((n_rec, 2), torch.int32), z(max_segs, torch.int64), z(15, torch.int64)
    en_sum = z(11, torch.int64)
    app_out = torch.empty(sb * cap, dtype=torch.uint8, device="cuda")   # one batch's recovery segments at a time
    app_certs, app_stat = z((sb, 2), torch.int32), z((sb, 2), torch.int32)
    names = segments.MIGRATE_SUMMARY_DTYPE.names
    as_dict = lambda t: {k: int(v) for k, v in zip(names, t.cpu().numpy().view(np.uint64))}
    en_names = segments.ENUMERATE_SUMMARY_DTYPE.names
    en_dict = lambda t: {k: int(v) for k, v in zip(en_names, t.cpu().numpy().view(np.uint64))}

    def live_append():
        for b in lst:
            p = parts[b]
            table.live(b, p.live, p.n_live, p.counts)
            ctx.recovery_append(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.live, p.n_live, 1,
                                app_out, cap, cap, app_certs, app_stat)

    results = {}
    for rname, last in RANGES.items():
        for mode in ("default", "live_only"):
            live = mode == "live_only"

            def migrate():
                table.migrate(lst, 0, out, cap, max_segs, certs, counts, summary, first_hash=0, last_hash=last,
                              live_only=live, sent=sent, sent_cap=n_rec, seg_first=seg_first)

            def enumerate_range(limit):
                """Every reply of the range into the copy's buffer; returns the objects seen."""
                bucket, nxt, seen = 0, 0, 0
                while True:
                    table.enumerate(0, copy_dst, en_sum, limit, first_hash=0, last_hash=last, bucket_index=bucket,
                                    bucket_next_hash=nxt, payload_capacity=limit)
                    s = en_dict(en_sum)
                    seen += s["objects"]
                    if not s["full"] or (s["next_bucket"] == bucket and s["next_hash"] == nxt):
                        return seen
                    bucket, nxt = s["next_bucket"], s["next_hash"]

            migrate()
            ctx.check()
            got = as_dict(summary)
            assert got["done"] == 1 and got["too_large"] == 0 and got["records_read"] == n_rec, got
            assert got["skipped_other"] == nseg and got["skipped_table"] == 0 and got["skipped_dead"] == 0, got
            assert got["sent_objects"] + got["skipped_range"] == n_obj and got["sent_tombstones"] == 0, got
            assert rname != "whole" or got["sent_objects"] == n_obj
            used = got["segments_used"]
            heads = certs[:used, 0].long() & 0xFFFFFFFF
            assert int(heads.sum().item()) == got["sent_bytes"] and int(counts[:used, 0].sum().item()) == got["sent_objects"]
            sb_bytes = got["sent_bytes"]
            en_limit = min(got["payload_bytes"] + 4 * got["sent_objects"] + 64, copy_dst.numel(), (1 << 32) - 64)
            assert enumerate_range(en_limit) == got["sent_objects"]
            ms = {w: [] for w in ("migrate", "copy", "enumerate")}
            with_la = live and rname == "whole"
            if with_la:
                ms["live_append"] = []
            for rnd in range(args.warmup + args.calls):
                t = dict(migrate=timed(migrate), copy=timed(lambda: copy_dst[:sb_bytes].copy_(out[:sb_bytes])),
                         enumerate=timed(lambda: enumerate_range(en_limit)))
                if with_la:
                    t["live_append"] = timed(live_append)
                if rnd >= args.warmup:
                    for w in ms:
                        ms[w].append(t[w])
            ctx.check()
            mmm = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
            ratios = {f"ratio_migrate_over_{w}_median_min_max": mmm([m / x for m, x in zip(ms["migrate"], ms[w])])
                      for w in ms if w != "migrate"}
            results[f"{rname}_{mode}"] = dict(
                summary=got, ms_median_min_max={w: mmm(v) for w, v in ms.items()},
                sent_gb_per_s_median=round(sb_bytes / float(np.median(ms["migrate"])) / 1e6, 1),
                scanned_records_per_us_median=round(n_rec / float(np.median(ms["migrate"])) / 1e3, 1), **ratios)
    tag = f"{nseg}x8MiB_b{nb}_v{value_len}"
    r = dict(value_len=value_len, nseg=nseg, batches=nb, segment_bytes=cap, records=n_rec, objects=n_obj,
             out_capacity=cap, max_segments=max_segs, calls_timed=args.calls, warmup=args.warmup,
             device=torch.cuda.get_device_name(0), build=ramcrc.lib().ramcrc_build_info().decode(), cases=results)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"migrate_{tag}.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                + "\n}\n")   # one key per line
    print(json.dumps({"replay_table_migrate": dict(
        tag=tag, **{s: dict(ms=v["ms_median_min_max"],
                            **{k[len("ratio_migrate_"):-len("_median_min_max")]: x for k, x in v.items()
                               if k.startswith("ratio_")},
                            sent_bytes=v["summary"]["sent_bytes"]) for s, v in results.items()})}), flush=True)
    table.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--values", type=lambda s: [int(v) for v in s.split(",") if v], default=[64, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5, help="timed rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_table_migrate"))
    ap.add_argument("--time-limit", type=int, default=240, help="seconds per value size")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        measure(args, int(args.child))
        return 0
    for line in [str(v) for v in args.values]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", line] + sys.argv[1:]
        try:
            rc = subprocess.run(cmd, timeout=args.time_limit).returncode
        except subprocess.TimeoutExpired:
            print("replay_table_migrate_bench: a GPU step exceeded its time limit", file=sys.stderr)
            return 124
        if rc:
            return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
