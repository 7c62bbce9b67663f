#!/usr/bin/env python3
"""Time an indexed read's reply from the replay table
(ramcrc_replay_table_read_hashes_device) beside the multi-read of the same keys
by key, and beside the lookup of the same keys plus a device-to-device copy of
exactly the reply's bytes.

    python tools/replay_table_read_hashes_bench.py [--nseg 512] [--batches 8]
                                                   [--values 64,1024,4096]
                                                   [--null-hashes] [--lines all,none,half]
                                                   [--out profiles/replay_table_read_hashes]

The table is replay_table_lookup_bench.py's: RecoverSegmentBenchmark-shaped
8 MiB segments built on the device (fill_objects: table 0, 8-byte counter
keys), the first entry of every segment retyped to a SEGHEADER, walked as
--batches batches and added batch by batch with the partition call's hashes.  A
second set of segments with later counter keys is walked but never added: its
hashes are the misses.

Three lines, n hashes each (n: the table's keys, in a shuffled order): `all`
present, `none`, and `half` (every second one a miss).  max_length and the
capacity hold everything.  In one round every line is timed three ways, each
bracketed by device events: the indexed read (d_parts NULL); the multi-read of
the same keys by key (default mode, hashes given, no rules, d_part_off and
d_results NULL); and the lookup of the same keys (hashes given, with counts)
plus a copy of the indexed read's reply_bytes (torch's copy_ of uint8 tensors,
which issues hipMemcpyAsync).  The ratios read_hashes / read and read_hashes /
(lookup + copy) are taken round by round, and the medians are over --calls
rounds after --warmup warm-up rounds.  Every timed call's summary is checked,
and once per line a call with d_parts checks 256 sampled hashes against the
lookup's results and the segment bytes.

--null-hashes adds one measurement per value size of a table whose batches were
added without hashes, where every claimant on a chain is hashed again in the
call: the `all` line only, next to the same line with hashes.

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
ALL_LINES = ("all", "none", "half")


def measure(args, value_len):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments
    from replay_table_bench import Walk

    LINES = tuple(args.lines)
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_table_read_hashes_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg, nb = 8 * MiB, args.nseg, args.batches
    assert nseg % nb == 0
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")

    def source(first_key):
        d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
        d.random_(0, 256)
        dc = z((nseg, 2), torch.int32)
        per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, value_len, first_key=first_key, certs=dc)
        first = d.view(nseg, cap)[:, 0]
        first.copy_((first & 0xC0) | segments.LOG_ENTRY_TYPE_SEGHEADER)
        ctx.certify(d, cap, cap, nseg, torch.full((nseg,), seg_len, dtype=torch.int32, device="cuda"), dc)
        parts = [Walk(torch, ctx, segments, d, dc, cap, b * (nseg // nb), nseg // nb, per) for b in range(nb)]
        for p in parts:
            p.walk(ctx)
        return d, per, parts

    def keys_of(parts):
        """(key bytes uint8 [n, 8], hashes int64 [n]) of the objects."""
        out = [[], []]
        for p in parts:
            n = int(p.n_entries.item())
            e = p.entries[:n].long()
            rec = torch.nonzero((e[:, 3] & 0x3F) == segments.LOG_ENTRY_TYPE_OBJ).reshape(-1)
            e = e[rec]
            at = e[:, 0] * cap + e[:, 1] + 1 + ((e[:, 3] >> 6) & 3) + 1 + 27
            out[0].append(p.d[at[:, None] + torch.arange(8, device="cuda")])
            out[1].append(p.key_hash[rec])
        return [torch.cat(x) for x in out]

    d, per, parts = source(0)
    d2, _, others = source(nseg * per)
    hit_key, hit_hash = keys_of(parts)
    miss_key, miss_hash = keys_of(others)
    del d2, others
    n = hit_key.shape[0]
    assert n == nseg * (per - 1) == miss_key.shape[0], (n, nseg, per)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    perm = torch.randperm(n, device="cuda", generator=g)
    hit_key, hit_hash, miss_key, miss_hash = hit_key[perm], hit_hash[perm], miss_key[perm], miss_hash[perm]
    even = torch.arange(n, device="cuda") % 2 == 0
    keybuf = {"all": hit_key, "none": miss_key, "half": torch.where(even[:, None], hit_key, miss_key)}
    hashes = {"all": hit_hash, "none": miss_hash, "half": torch.where(even, hit_hash, miss_hash)}
    keybuf = {k: v.contiguous().reshape(-1) for k, v in keybuf.items()}
    hashes = {k: v.contiguous() for k, v in hashes.items()}
    present = {"all": n, "none": 0, "half": (n + 1) // 2}
    queries = z((n, 3), torch.int64)   # table 0, key_off, key_len 8 (reserved 0)
    queries[:, 1] = 8 * torch.arange(n, device="cuda")
    queries[:, 2] = 8
    kv = 1 + 2 + 8 + value_len   # key count, one cumulative length, the key, the value
    reply = torch.empty(n * (16 + kv), dtype=torch.uint8, device="cuda")   # (the multi-read's is the longer)
    copy_dst = torch.empty(n * (12 + kv), dtype=torch.uint8, device="cuda")
    rh_summary, rd_summary = z(9, torch.int64), z(10, torch.int64)
    results = z((n, 8), torch.int32)
    counts = z(5, torch.int64)
    hparts = z((n, 2), torch.int64)
    tiles = (n + 255) // 256
    ctx.reserve(32 + 16 * tiles, max(6 * n, max(p.ecap for p in parts)))
    table = ramcrc.ReplayTable(ctx, nseg * per, nb)

    def adds(given):
        table.reset()
        for p in parts:
            table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work,
                      key_hash=p.key_hash if given else None)
        ctx.check()

    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def want_rh(line):
        ok = present[line]
        return dict(hashes=n, objects=ok, objects_counted=ok, reply_bytes=ok * (12 + kv), value_bytes=ok * value_len,
                    key_bytes=ok * 11, empty=n - ok, tombstones=0, spoiled=0)

    def got(summary, dt):
        s = summary.cpu().numpy().view(dt)[0]
        return {k: int(s[k]) for k in dt.names}

    def read_hashes(line, with_parts=False):
        table.read_hashes(0, hashes[line], reply, rh_summary, 1 << 62, parts=hparts if with_parts else None)

    sample = torch.randint(0, n, (256,), device="cuda", generator=g)

    def check_parts(line):
        """256 sampled hashes against the lookup's results and the segment bytes."""
        read_hashes(line, True)
        assert got(rh_summary, segments.READ_HASHES_SUMMARY_DTYPE) == want_rh(line)
        table.lookup(keybuf[line], queries, results, counts=counts, key_hash=hashes[line])
        r = results[sample].cpu().numpy().view(segments.LOOKUP_RESULT_DTYPE).reshape(-1)
        hp = hparts[sample].cpu().numpy().view(segments.HASH_PART_DTYPE).reshape(-1)
        base = np.cumsum([0] + [p.nseg for p in parts[:-1]])
        for q, res, part in zip(sample.tolist(), r, hp):
            if res["kind"] != segments.LOOKUP_OBJECT:
                assert line != "all" and int(part["objects"]) == 0, (q, part)
                continue
            off = int(part["off"])
            head = reply[off:off + 12].cpu().numpy().view(segments.READ_HASHES_OBJECT_DTYPE)[0]
            at = (int(base[res["batch"]]) + int(res["segment"])) * cap + int(res["value_off"]) - 11
            assert int(part["objects"]) == 1 and tuple(head.tolist()) == (int(res["version"]), kv), (q, head)
            assert torch.equal(reply[off + 12:off + 12 + kv], d[at:at + kv]), q

    def one_round(line):
        t_rh = timed(lambda: read_hashes(line))
        want = want_rh(line)
        assert got(rh_summary, segments.READ_HASHES_SUMMARY_DTYPE) == want
        rb = want["reply_bytes"]
        t_look = timed(lambda: table.lookup(keybuf[line], queries, results, counts=counts, key_hash=hashes[line]))
        t_copy = timed(lambda: copy_dst[:rb].copy_(reply[:rb]))
        t_read = timed(lambda: table.read(keybuf[line], queries, reply, rd_summary, key_hash=hashes[line]))
        s = got(rd_summary, segments.READ_SUMMARY_DTYPE)
        assert s["returned"] == n and s["ok"] == present[line] and s["reply_bytes"] == 16 * n + present[line] * kv, s
        return t_rh, t_read, t_look, t_copy

    WHAT = ("read_hashes", "read", "lookup", "copy")
    mmm = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
    null = None
    if args.null_hashes:
        # every claimant on a chain is hashed again in the call: the price of the missing hashes
        adds(False)
        for _ in range(args.warmup):
            read_hashes("all")
        check_parts("all")
        null = mmm([timed(lambda: read_hashes("all")) for _ in range(args.calls)])
    adds(True)
    for _ in range(args.warmup):
        for line in LINES:
            one_round(line)
    ctx.check()
    for line in LINES:
        check_parts(line)
    ms = {f"{line}_{what}": [] for line in LINES for what in WHAT}
    for _ in range(args.calls):   # alternate, so that none has the quieter part of the run
        for line in LINES:
            for what, t in zip(WHAT, one_round(line)):
                ms[f"{line}_{what}"].append(t)
    ctx.check()
    per_round = lambda line, f: [f(*x) for x in zip(*(ms[f"{line}_{w}"] for w in WHAT))]
    over_read = {line: mmm(per_round(line, lambda rh, rd, lk, c: rh / rd)) for line in LINES}
    over_lookup_copy = {line: mmm(per_round(line, lambda rh, rd, lk, c: rh / (lk + c))) for line in LINES}
    # the read's own spread between rounds: (max - min) / median
    read_spread = {line: round((max(ms[line + "_read"]) - min(ms[line + "_read"])) /
                               float(np.median(ms[line + "_read"])), 4) for line in LINES}
    r = {"value_len": value_len, "nseg": nseg, "batches": nb, "segment_bytes": cap, "keys": n, "hashes": n,
         "reply_bytes": {line: want_rh(line)["reply_bytes"] for line in LINES},
         "calls_timed": args.calls, "warmup": args.warmup,
         "device": torch.cuda.get_device_name(0), "build": ramcrc.lib().ramcrc_build_info().decode(),
         "ms_median_min_max": {k: mmm(v) for k, v in ms.items()},
         "ms_rounds": {k: [round(x, 4) for x in v] for k, v in ms.items()},
         "ratio_read_hashes_over_read_median_min_max": over_read,
         "ratio_read_hashes_over_lookup_plus_copy_median_min_max": over_lookup_copy,
         "read_spread_over_median": read_spread}
    if null is not None:
        r["null_hashes_all_read_hashes_ms_median_min_max"] = null
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"read_hashes_{nseg}x8MiB_b{nb}_v{value_len}.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                + "\n}\n")   # one key per line
    print(json.dumps({"replay_table_read_hashes": dict(
        value_len=value_len, keys=n, over_read=over_read, over_lookup_plus_copy=over_lookup_copy,
        read_spread=read_spread, null_hashes_all_ms=null,
        **{k + "_ms": r["ms_median_min_max"][k] for k in ms})}), flush=True)
    table.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--values", type=lambda s: [int(v) for v in s.split(",")], default=[64, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=15, help="timed rounds")
    ap.add_argument("--lines", type=lambda s: s.split(","), default=list(ALL_LINES),
                    help="the lines to time (for a kernel trace of one of them)")
    ap.add_argument("--null-hashes", action="store_true",
                    help="also time the `all` line on a table added without hashes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_table_read_hashes"))
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
            print("replay_table_read_hashes_bench: a GPU step exceeded its time limit", file=sys.stderr)
            return 124
        if rc:
            return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
