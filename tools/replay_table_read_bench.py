#!/usr/bin/env python3
"""Time a multi-read's reply from the replay table
(ramcrc_replay_table_read_device) beside the lookup of the same queries and a
device-to-device copy of exactly the reply's bytes.

    python tools/replay_table_read_bench.py [--nseg 512] [--batches 8]
                                            [--values 64,1024,4096]
                                            [--out profiles/replay_table_read]

The table is replay_table_lookup_bench.py's: RecoverSegmentBenchmark-shaped
8 MiB segments built on the device (fill_objects: table 0, 8-byte counter
keys), the first entry of every segment retyped to a SEGHEADER, walked as
--batches batches and added batch by batch.  A second set of segments with later
counter keys is walked but never added: its keys are the misses.

Three lines, n queries each (n: the table's keys, in a shuffled order):
`keys_and_value` and `value_only`, every key present, in the two modes; and
`tenth_absent`, keys and values with every tenth key replaced by one the table
does not hold.  reply_cap holds everything.  In one round every line is timed
three ways, each bracketed by device events: the read (hashes computed in the
call, no rules, d_part_off and d_results NULL); the lookup of the same queries
(hashes computed, with counts); and a copy of the reply's reply_bytes (torch's
copy_ of uint8 tensors, which issues hipMemcpyAsync).  The yardstick of a read
is lookup + copy of the same round; the ratio read / (lookup + copy) is taken
round by round, and the medians are over --calls rounds after --warmup warm-up
rounds.  Every timed read's summary is checked, and once per line a read with
d_part_off and d_results checks 256 sampled parts against the lookup's results
and the segment bytes.  One JSON file per value size, and one summary line each
on stdout.

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
LINES = (("keys_and_value", False, False), ("value_only", True, False), ("tenth_absent", False, True))


def measure(args, value_len):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments
    from replay_table_bench import Walk

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_table_read_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
    cap, nseg, nb = 8 * MiB, args.nseg, args.batches
    assert nseg % nb == 0
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")

    def source(first_key, count):
        d = torch.empty(count * cap, dtype=torch.uint8, device="cuda")
        d.random_(0, 256)
        dc = z((count, 2), torch.int32)
        per, seg_len, _ = ctx.fill_objects(d, cap, cap, count, value_len, first_key=first_key, certs=dc)
        first = d.view(count, cap)[:, 0]
        first.copy_((first & 0xC0) | segments.LOG_ENTRY_TYPE_SEGHEADER)
        ctx.certify(d, cap, cap, count, torch.full((count,), seg_len, dtype=torch.int32, device="cuda"), dc)
        k = nb if count == nseg else 1
        parts = [Walk(torch, ctx, segments, d, dc, cap, b * (count // k), count // k, per) for b in range(k)]
        for p in parts:
            p.walk(ctx)
        return d, per, parts

    def keys_of(parts):
        out = []
        for p in parts:
            n = int(p.n_entries.item())
            e = p.entries[:n].long()
            e = e[(e[:, 3] & 0x3F) == segments.LOG_ENTRY_TYPE_OBJ]
            at = e[:, 0] * cap + e[:, 1] + 1 + ((e[:, 3] >> 6) & 3) + 1 + 27
            out.append(p.d[at[:, None] + torch.arange(8, device="cuda")])
        return torch.cat(out)

    d, per, parts = source(0, nseg)
    hit_key = keys_of(parts)
    n = hit_key.shape[0]
    assert n == nseg * (per - 1), (n, nseg, per)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    hit_key = hit_key[torch.randperm(n, device="cuda", generator=g)]
    # the misses: a tenth of n keys from segments that are never added
    n_miss = (n + 9) // 10
    miss_seg = (n_miss + per - 2) // (per - 1)
    d2, _, others = source(nseg * per, miss_seg)
    miss_key = keys_of(others)[:n_miss]
    del d2, others
    tenth = torch.arange(n, device="cuda") % 10 == 0
    mixed_key = hit_key.clone()
    mixed_key[tenth] = miss_key[:int(tenth.sum())]
    keybuf = {False: hit_key.contiguous().reshape(-1), True: mixed_key.contiguous().reshape(-1)}
    queries = z((n, 3), torch.int64)   # table 0, key_off, key_len 8 (reserved 0)
    queries[:, 1] = 8 * torch.arange(n, device="cuda")
    queries[:, 2] = 8
    kv = 1 + 2 + 8 + value_len   # key count, one cumulative length, the key, the value
    room = n * (16 + kv)
    reply = torch.empty(room, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty(room, dtype=torch.uint8, device="cuda")
    summary = z(10, torch.int64)
    results = z((n, 8), torch.int32)
    counts = z(5, torch.int64)
    part_off = z(n, torch.int64)
    ctx.reserve(32 + 8 * ((n + 255) // 256), max(4 * n, max(p.ecap for p in parts)))
    table = ramcrc.ReplayTable(ctx, nseg * per, nb)
    for p in parts:
        table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work, key_hash=None)
    ctx.check()
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def want_summary(value_only, absent):
        miss = int(tenth.sum()) if absent else 0
        ok = n - miss
        return dict(returned=n, reply_bytes=16 * n + ok * (value_len if value_only else kv), ok=ok,
                    doesnt_exist=miss, object_exists=0, wrong_version=0, bad=0, value_bytes=ok * value_len,
                    key_bytes=ok * 11, spoiled=0)

    def got_summary():
        s = summary.cpu().numpy().view(segments.READ_SUMMARY_DTYPE)[0]
        return {k: int(s[k]) for k in segments.READ_SUMMARY_DTYPE.names}

    sample = torch.randint(0, n, (256,), device="cuda", generator=g)

    def check_parts(value_only, absent):
        """256 sampled parts against the lookup's results and the segment bytes."""
        table.read(keybuf[absent], queries, reply, summary, value_only=value_only, part_off=part_off,
                   results=results)
        assert got_summary() == want_summary(value_only, absent), got_summary()
        looked = torch.zeros_like(results)
        table.lookup(keybuf[absent], queries, looked, counts=counts)
        assert torch.equal(looked, results), "d_results differs from the lookup's"
        r = results[sample].cpu().numpy().view(segments.LOOKUP_RESULT_DTYPE).reshape(-1)
        offs = part_off[sample].cpu().numpy()
        base = np.cumsum([0] + [p.nseg for p in parts[:-1]])
        for q, res, off in zip(sample.tolist(), r, offs.tolist()):
            head = reply[off:off + 16].cpu().numpy().view(segments.READ_PART_DTYPE)[0]
            if res["kind"] != segments.LOOKUP_OBJECT:
                assert absent and q % 10 == 0 and tuple(head.tolist()) == (3, 0, 0), (q, head)
                continue
            at = (int(base[res["batch"]]) + int(res["segment"])) * cap + int(res["value_off"])
            at, ln = (at, value_len) if value_only else (at - 11, kv)
            assert tuple(head.tolist()) == (0, int(res["version"]), ln), (q, head)
            assert torch.equal(reply[off + 16:off + 16 + ln], d[at:at + ln]), q

    def one_round(value_only, absent):
        t_read = timed(lambda: table.read(keybuf[absent], queries, reply, summary, value_only=value_only))
        want = want_summary(value_only, absent)
        assert got_summary() == want, got_summary()
        t_look = timed(lambda: table.lookup(keybuf[absent], queries, results, counts=counts))
        rb = want["reply_bytes"]
        t_copy = timed(lambda: copy_dst[:rb].copy_(reply[:rb]))
        return t_read, t_look, t_copy

    for _ in range(args.warmup):
        for _, value_only, absent in LINES:
            one_round(value_only, absent)
    ctx.check()
    for _, value_only, absent in LINES:
        check_parts(value_only, absent)
    ms = {f"{name}_{what}": [] for name, _, _ in LINES for what in ("read", "lookup", "copy")}
    for _ in range(args.calls):   # alternate, so that none has the quieter part of the run
        for name, value_only, absent in LINES:
            for what, t in zip(("read", "lookup", "copy"), one_round(value_only, absent)):
                ms[f"{name}_{what}"].append(t)
    ctx.check()
    mmm = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
    ratio = {name: mmm([r / (lk + c) for r, lk, c in zip(ms[name + "_read"], ms[name + "_lookup"],
                                                          ms[name + "_copy"])]) for name, _, _ in LINES}
    r = {"value_len": value_len, "nseg": nseg, "batches": nb, "segment_bytes": cap, "keys": n, "queries": n,
         "reply_bytes": {name: want_summary(vo, ab)["reply_bytes"] for name, vo, ab in LINES},
         "calls_timed": args.calls, "warmup": args.warmup,
         "device": torch.cuda.get_device_name(0), "build": ramcrc.lib().ramcrc_build_info().decode(),
         "ms_median_min_max": {k: mmm(v) for k, v in ms.items()},
         "reply_gb_per_s_median": {name: round(want_summary(vo, ab)["reply_bytes"] /
                                               float(np.median(ms[name + "_read"])) / 1e6, 1)
                                   for name, vo, ab in LINES},
         # per round: the read over the lookup of the same queries plus the copy of the reply
         "ratio_read_over_lookup_plus_copy_median_min_max": ratio}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"read_{nseg}x8MiB_b{nb}_v{value_len}.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                + "\n}\n")   # one key per line
    print(json.dumps({"replay_table_read": dict(value_len=value_len, keys=n, ratio=ratio,
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
    ap.add_argument("--calls", type=int, default=15, help="timed rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_table_read"))
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
            print("replay_table_read_bench: a GPU step exceeded its time limit", file=sys.stderr)
            return 124
        if rc:
            return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
