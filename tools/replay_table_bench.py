#!/usr/bin/env python3
"""Time the replay table (ramcrc_replay_table_*), fed batch by batch, beside
the one-call ramcrc_replay_resolve_device over the same segments and a
device-to-device copy of the same bytes.

    python tools/replay_table_bench.py [--nseg 512] [--batches 8]
                                       [--values 64,1024,4096]
                                       [--out profiles/replay_table]

Sources are RecoverSegmentBenchmark-shaped 8 MiB segments built on the device
(fill_objects: table 0, 8-byte counter keys, version 0), the first entry of
every segment retyped to a SEGHEADER as in replay_resolve_bench.py.  Two shapes
per value size: `distinct` (every key once) and `twice` (the second half of the
segments are byte copies of the first half, so the later batches bring every
key a second time and the earlier batch's record stays the winner).

The segments are walked twice before anything is timed: once as a whole, for
the one-call, and once as --batches batches of nseg / batches segments with
tables of their own, for the table (the partition call supplies each table's
hashes).  In one run the calls alternate -- the table with the given hashes
(reset, the adds, then one live query per batch), the table with NULL hashes,
the one-call with given and with NULL hashes, the copy (torch's copy_ of uint8
tensors, which issues hipMemcpyAsync) -- each bracketed by device events; the
medians are over --calls calls after --warmup warm-up rounds.  The table's time
is the sum of its adds and live queries; the reset before them is timed by
itself.  One JSON file per value size and shape, and one summary line each on
stdout.

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


class Walk:
    """A walk's tables over segments [lo, lo + nseg) with the partition call's hashes."""

    def __init__(self, torch, ctx, segments, d, dc, cap, lo, nseg, per):
        self.d, self.nseg = d[lo * cap:(lo + nseg) * cap], nseg
        self.dc = dc[lo:lo + nseg]
        ecap = self.ecap = nseg * (per + 1)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.status, self.entries = z((nseg, 4), torch.int32), z((ecap, 4), torch.int32)
        self.n_entries, self.key_hash = z(1, torch.int64), z(ecap, torch.int64)
        self.place, self.n_place, self.pstat = z((ecap, 2), torch.int32), z(1, torch.int64), z((nseg, 4), torch.int32)
        self.live, self.n_live, self.counts = z((ecap, 2), torch.int32), z(1, torch.int64), z(6, torch.int64)
        self.work = z(ecap, torch.int64)
        self.tabs = segments.tablets_tensor([(0, 0, (1 << 64) - 1, 0, 0, 0)])
        self.cap = cap

    def walk(self, ctx):
        ctx.segment_walk(self.d, self.cap, self.cap, self.nseg, self.dc, self.status, self.entries,
                         self.n_entries)
        ctx.recovery_partition(self.d, self.cap, self.nseg, self.status, self.entries, self.n_entries,
                               self.tabs, 1, self.place, self.n_place, self.pstat,
                               key_hash=self.key_hash, n_tablets=1)


def measure(args, value_len):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_table_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg, nb = 8 * MiB, args.nseg, args.batches
    assert nseg % nb == 0 and (nb % 2 == 0 or nb == 1)
    d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    d.random_(0, 256)
    dc = torch.zeros((nseg, 2), dtype=torch.int32, device="cuda")
    per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, value_len, certs=dc)
    first = d.view(nseg, cap)[:, 0]
    first.copy_((first & 0xC0) | segments.LOG_ENTRY_TYPE_SEGHEADER)
    heads = torch.full((nseg,), seg_len, dtype=torch.int32, device="cuda")
    ctx.certify(d, cap, cap, nseg, heads, dc)
    whole = Walk(torch, ctx, segments, d, dc, cap, 0, nseg, per)
    parts = [Walk(torch, ctx, segments, d, dc, cap, b * (nseg // nb), nseg // nb, per) for b in range(nb)]
    winner = torch.zeros(whole.ecap, dtype=torch.int32, device="cuda")
    copy_dst = torch.empty(nseg * seg_len, dtype=torch.uint8, device="cuda")
    stats = torch.zeros(6, dtype=torch.int64, device="cuda")
    ctx.reserve(16 + 6 * slots_for(whole.ecap), 2 * whole.ecap)
    table = ramcrc.ReplayTable(ctx, whole.ecap, nb)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def resolve(hashes):
        ctx.replay_resolve(d, cap, nseg, whole.status, whole.entries, whole.n_entries, whole.live,
                           whole.n_live, whole.counts, key_hash=hashes, winner=winner)

    def run_table(given):
        """(reset ms, adds ms, lives ms)"""
        e = [ev() for _ in range(4)]
        e[0].record()
        table.reset()
        e[1].record()
        for p in parts:
            table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work,
                      key_hash=p.key_hash if given else None)
        e[2].record()
        for b, p in enumerate(parts):
            table.live(b, p.live, p.n_live, p.counts)
        e[3].record()
        e[3].synchronize()
        return [e[k].elapsed_time(e[k + 1]) for k in range(3)]

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    src = d[:nseg * seg_len]
    for shape in ("distinct", "twice"):
        if shape == "twice":
            half = nseg // 2
            d.view(nseg, cap)[half:2 * half].copy_(d.view(nseg, cap)[:half])
            dc[half:2 * half].copy_(dc[:half])
        for w in [whole] + parts:
            w.walk(ctx)
        for _ in range(args.warmup):
            run_table(True)
            run_table(False)
            resolve(whole.key_hash)
            resolve(None)
            copy_dst.copy_(src)
        ctx.check()
        # the table's verdicts are the one-call's: the same number of records kept,
        # batch by batch the one-call's live records of those segments
        n, kept = int(whole.n_entries.item()), int(whole.n_live.item())
        ct = whole.counts.cpu().numpy().view(segments.RESOLVE_COUNTS_DTYPE)[0]
        keys = n - nseg if shape == "distinct" else (n - nseg) - (nseg // 2) * (per - 1)
        assert n == nseg * per and kept == keys == int(ct["live_objects"]), (shape, n, kept, keys, ct)
        table.stats(stats)
        st = stats.cpu().numpy().view(segments.REPLAY_TABLE_STATS_DTYPE)[0]
        assert (int(st["keys"]), int(st["live_objects"]), int(st["batches"]), int(st["spoiled"])) == \
            (keys, keys, nb, 0), st
        kept_by_batch = [int(p.n_live.item()) for p in parts]
        assert sum(kept_by_batch) == kept, (kept_by_batch, kept)
        if shape == "twice":
            # (the one-call keeps whichever twin the walk listed first; the table the earlier batch's)
            assert not any(kept_by_batch[nb // 2:]), kept_by_batch
        else:
            one_live_seg = whole.entries[whole.live[:kept, 0].long(), 0].long()
            for b, p in enumerate(parts):
                lo = b * (nseg // nb)
                assert int(((one_live_seg >= lo) & (one_live_seg < lo + p.nseg)).sum()) == kept_by_batch[b]

        names = ["table_given", "table_null", "resolve_given", "resolve_null", "memcpy"]
        ms = {k: [] for k in names}
        detail = {k: {"reset": [], "adds": [], "lives": []} for k in ("table_given", "table_null")}
        for _ in range(args.calls):   # alternate, so that none has the quieter part of the run
            for k in names:
                if k.startswith("table"):
                    r, a, l = run_table(k == "table_given")
                    ms[k].append(a + l)
                    for name, v in zip(("reset", "adds", "lives"), (r, a, l)):
                        detail[k][name].append(v)
                elif k == "memcpy":
                    ms[k].append(timed(lambda: copy_dst.copy_(src)))
                else:
                    ms[k].append(timed(lambda: resolve(whole.key_hash if k == "resolve_given" else None)))
        ctx.check()
        assert [int(p.n_live.item()) for p in parts] == kept_by_batch
        mmm = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
        ratio = lambda a, b: mmm([x / y for x, y in zip(ms[a], ms[b])])
        r = {"shape": shape, "value_len": value_len, "nseg": nseg, "batches": nb, "segment_bytes": cap,
             "records": n, "participants": n - nseg, "live": kept, "live_by_batch": kept_by_batch,
             "table_slots": slots_for(whole.ecap), "one_call_slots": slots_for(n),
             "segment_bytes_used": nseg * seg_len,
             "calls_timed": args.calls, "warmup": args.warmup,
             "device": torch.cuda.get_device_name(0), "build": ramcrc.lib().ramcrc_build_info().decode(),
             "ms_median_min_max": {k: mmm(v) for k, v in ms.items()},
             "table_parts_ms_median_min_max": {k: {p: mmm(v) for p, v in d_.items()}
                                               for k, d_ in detail.items()},
             # per round: the table's adds and live queries over the one-call of the same round
             "ratio_table_over_one_call_median_min_max": {"given": ratio("table_given", "resolve_given"),
                                                          "null": ratio("table_null", "resolve_null")}}
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, f"table_{nseg}x8MiB_b{nb}_v{value_len}_{shape}.json"), "w") as f:
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                    + "\n}\n")   # one key per line
        print(json.dumps({"replay_table": dict(shape=shape, value_len=value_len, records=n, live=kept,
                                               ratio=r["ratio_table_over_one_call_median_min_max"],
                                               **{k + "_ms": r["ms_median_min_max"][k] for k in ms})}),
              flush=True)
    table.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--values", type=lambda s: [int(v) for v in s.split(",")], default=[64, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=15, help="timed calls of each kind, alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_table"))
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
            print("replay_table_bench: a GPU step exceeded its time limit", file=sys.stderr)
            return 124
        if rc:
            return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
