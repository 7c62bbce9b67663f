#!/usr/bin/env python3
"""Time a multi-remove against the replay table
(ramcrc_replay_table_remove_device) beside its parts: the lookup of the same
keys and a device-to-device copy of exactly the output's bytes.

    python tools/replay_table_remove_bench.py [--nseg 512] [--batches 8]
                                              [--values 64,1024,4096]
                                              [--long-keys 4194304]
                                              [--out profiles/replay_table_remove]

The table is replay_table_write_bench.py's: RecoverSegmentBenchmark-shaped
8 MiB segments built on the device (fill_objects: table 0, 8-byte counter
keys), the first entry of every segment retyped to a SEGHEADER, walked as
--batches batches and added batch by batch, every object's version set to 1
before the add.

The requests are as many 8-byte keys as the table holds, in a shuffled order.
Three shapes: `all_present` (table 0: one 42-byte tombstone entry each),
`none_present` (the same keys under table 1: nothing is written) and `half`
(alternating).  In one round every shape is timed three ways, each bracketed
by device events: the remove (hashes computed in the call, no rules, d_refs,
d_old and d_batch_segment_id NULL); the lookup of the same keys in the same
buffer (hashes computed, with counts); and a copy of the output's out_bytes
(torch's copy_ of uint8 tensors, which issues hipMemcpyAsync).  The yardstick
of a remove is lookup + copy of the same round; the ratio remove / (lookup +
copy) is taken round by round, and the medians are over --calls rounds after
--warmup warm-up rounds.  Every timed remove's summary is checked, and once per
shape a remove with d_refs checks 256 sampled requests: the entry header, the
tombstone's fields, its key and its checksum against the host CRC.  The
certificate is not walked here; the tests do that.  One JSON file per value
size, and one summary line each on stdout.

One further line, `keys64`, removes --long-keys 64-byte keys, every one
present: the table for it is made by the project's own write call (64
segments of one-key objects with 64-byte keys and 64-byte values, written
against an empty table, walked with the write's certificates and added as one
batch), so the tombstones are 98-byte entries written by groups of 8 lanes.

Each line is measured in a child process of its own under a time limit; this
process never opens the GPU.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
SHAPES = ("all_present", "none_present", "half")
TS = 0x7E40BE5D


def run_shapes(args, np, torch, ramcrc, segments, ctx, table, keys, key_len, table_of, shapes, tag, extra,
               version_of):
    """Time `shapes` over the keys (uint8 [n, key_len]) and write the JSON;
    version_of(q): the version of request q's object."""
    n = keys.shape[0]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    ar = lambda k: torch.arange(k, device="cuda")
    kb = keys.reshape(-1).contiguous()
    tlen = 32 + key_len
    entry = 2 + tlen
    assert tlen < 256
    reqs = {}
    for name in shapes:
        r = z((n, 3), torch.int64)
        r[:, 0], r[:, 1], r[:, 2] = table_of[name], key_len * ar(n), key_len
        reqs[name] = r
    present = {name: int((table_of[name] == 0).sum()) for name in shapes}
    out_bytes = {name: present[name] * entry for name in shapes}
    room = max(max(out_bytes.values()), 16)
    assert room < 1 << 32
    out = torch.empty(room, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty(room, dtype=torch.uint8, device="cuda")
    cert, summary = z(2, torch.int32), z(12, torch.int64)
    rparts = z(3 * n, torch.int32)
    refs = z(n, torch.int32)
    results, counts = z((n, 8), torch.int32), z(5, torch.int64)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    nv = 1 << 40
    names = segments.REMOVE_SUMMARY_DTYPE.names

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def want_summary(name):
        p = present[name]
        return dict(dict.fromkeys(names, 0), removed=p, ok_absent=n - p, next_version=nv, out_bytes=out_bytes[name],
                    tombstone_bytes=p * tlen)

    def got_summary():
        s = summary.cpu().numpy().view(segments.REMOVE_SUMMARY_DTYPE)[0]
        return {k: int(s[k]) for k in names}

    def remove(name, with_refs=False):
        table.remove(kb, reqs[name], out, cert, rparts, summary, nv, TS, refs=refs if with_refs else None,
                     out_capacity=out_bytes[name])

    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    sample = torch.randint(0, n, (256,), device="cuda", generator=g)

    def check(name):
        """256 sampled requests against the host CRC."""
        remove(name, True)
        assert got_summary() == want_summary(name), got_summary()
        r = refs.cpu().numpy().view(np.uint32)
        pp = rparts.cpu().numpy().view(np.uint8).reshape(n, 12)
        for q in sample.tolist():
            tid = int(table_of[name][q].item())
            status, version = int.from_bytes(pp[q, :4].tobytes(), "little"), int.from_bytes(pp[q, 4:].tobytes(), "little")
            assert status == 0, q
            if tid != 0:
                assert int(r[q]) == 0xFFFFFFFF and version == 0, q
                continue
            at = int(r[q])
            t = out[at:at + entry].cpu().numpy().tobytes()
            assert version == version_of(q) and t[0] == segments.LOG_ENTRY_TYPE_OBJTOMB and t[1] == tlen, q
            tp = t[2:]
            assert tp[:8] == bytes(8) and tp[8:16] == bytes(8) and tp[16:24] == version.to_bytes(8, "little"), q
            assert tp[24:28] == TS.to_bytes(4, "little") and tp[32:] == keys[q].cpu().numpy().tobytes(), q
            assert int.from_bytes(tp[28:32], "little") == ramcrc.crc32c(tp[:28] + tp[32:]), q

    def one_round(name):
        t_remove = timed(lambda: remove(name))
        assert got_summary() == want_summary(name), got_summary()
        t_look = timed(lambda: table.lookup(kb, reqs[name], results, counts=counts))
        ob = out_bytes[name]
        t_copy = timed(lambda: copy_dst[:ob].copy_(out[:ob]))
        return t_remove, t_look, t_copy

    for name in shapes:
        check(name)
    ctx.check()
    for _ in range(args.warmup):
        for name in shapes:
            one_round(name)
    ctx.check()
    whats = ("remove", "lookup", "copy")
    ms = {f"{name}_{what}": [] for name in shapes for what in whats}
    for _ in range(args.calls):   # alternate, so that none has the quieter part of the run
        for name in shapes:
            for what, t in zip(whats, one_round(name)):
                ms[f"{name}_{what}"].append(t)
    ctx.check()
    mmm = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
    ratio = {name: mmm([w / (lk + c) for w, lk, c in zip(*(ms[f"{name}_{x}"] for x in whats))]) for name in shapes}
    r = dict(extra, key_len=key_len, requests=n, out_bytes=out_bytes, calls_timed=args.calls, warmup=args.warmup,
             device=torch.cuda.get_device_name(0), build=ramcrc.lib().ramcrc_build_info().decode(),
             ms_median_min_max={k: mmm(v) for k, v in ms.items()},
             requests_per_us_median={name: round(n / float(np.median(ms[name + "_remove"])) / 1e3, 2)
                                     for name in shapes},
             # per round: the remove over the lookup of the same keys and the copy of the output
             ratio_remove_over_lookup_plus_copy_median_min_max=ratio)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"remove_{tag}.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                + "\n}\n")   # one key per line
    print(json.dumps({"replay_table_remove": dict(tag=tag, key_len=key_len, requests=n, ratio=ratio,
                                                  **{k + "_ms": r["ms_median_min_max"][k] for k in ms})}),
          flush=True)


def setup(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_table_remove_bench: no GPU (no fallback)")
    return np, torch, ramcrc, segments, ramcrc.Context(0)


def slots_for(n):
    slots = 64
    while slots < 2 * n:
        slots *= 2
    return slots


def measure(args, value_len):
    np, torch, ramcrc, segments, ctx = setup(args)
    from replay_table_bench import Walk
    cap, nseg, nb = 8 * MiB, args.nseg, args.batches
    assert nseg % nb == 0
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    ar = lambda k: torch.arange(k, device="cuda")

    d = torch.empty(nseg * cap, dtype=torch.uint8, device="cuda")
    d.random_(0, 256)
    dc = z((nseg, 2), torch.int32)
    per, seg_len, _ = ctx.fill_objects(d, cap, cap, nseg, value_len, first_key=0, certs=dc)
    first = d.view(nseg, cap)[:, 0]
    first.copy_((first & 0xC0) | segments.LOG_ENTRY_TYPE_SEGHEADER)
    ctx.certify(d, cap, cap, nseg, torch.full((nseg,), seg_len, dtype=torch.int32, device="cuda"), dc)
    parts = [Walk(torch, ctx, segments, d, dc, cap, b * (nseg // nb), nseg // nb, per) for b in range(nb)]
    keys = []
    for p in parts:
        p.walk(ctx)
        e = p.entries[:int(p.n_entries.item())].long()
        e = e[(e[:, 3] & 0x3F) == segments.LOG_ENTRY_TYPE_OBJ]
        pay = e[:, 0] * cap + e[:, 1] + 1 + ((e[:, 3] >> 6) & 3) + 1
        p.d[pay + 8] = 1   # version 1
        keys.append(p.d[(pay + 27)[:, None] + ar(8)])
    keys = torch.cat(keys)
    n = keys.shape[0]
    assert n == nseg * (per - 1), (n, nseg, per)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    keys = keys[torch.randperm(n, device="cuda", generator=g)]
    table_of = {"all_present": z(n, torch.int64), "none_present": torch.ones(n, dtype=torch.int64, device="cuda"),
                "half": ar(n) % 2}
    ctx.reserve(32 + 10 * ((n + 255) // 256), max(5 * n + slots_for(n), max(p.ecap for p in parts)))
    table = ramcrc.ReplayTable(ctx, nseg * per, nb)
    for p in parts:
        table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work, key_hash=None)
    ctx.check()
    run_shapes(args, np, torch, ramcrc, segments, ctx, table, keys, 8, table_of, SHAPES,
               f"{nseg}x8MiB_b{nb}_v{value_len}",
               dict(value_len=value_len, nseg=nseg, batches=nb, segment_bytes=cap, keys=n), lambda q: 1)
    table.close()
    ctx.close()


def measure_long_keys(args):
    """The keys64 line: a table of 64-byte keys made by the write call."""
    np, torch, ramcrc, segments, ctx = setup(args)
    from replay_table_bench import Walk
    key_len, value_len, nseg = 64, 64, 64
    n = args.long_keys
    per = n // nseg
    assert per * nseg == n
    image = 1 + 2 + key_len + value_len
    entry = 1 + 1 + 24 + image
    cap = -(-(per * entry) // MiB) * MiB
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    ar = lambda k: torch.arange(k, device="cuda")
    data = torch.empty((n, image), dtype=torch.uint8, device="cuda")
    data.random_(0, 256)
    data[:, 0], data[:, 1], data[:, 2] = 1, key_len, 0
    data[:, 3:11] = ar(n).view(torch.uint8).reshape(n, 8)   # distinct keys
    keys = data[:, 3:3 + key_len].contiguous()
    data = data.reshape(-1)
    d = z(nseg * cap, torch.uint8)
    dc = z((nseg, 2), torch.int32)
    ctx.reserve(32 + 12 * ((n + 255) // 256), 8 * n + 2 * slots_for(n))
    empty = ramcrc.ReplayTable(ctx, 64, 1)
    wparts, wsum = z(3 * per, torch.int32), z(16, torch.int64)
    for s in range(nseg):
        r = z((per, 3), torch.int64)
        r[:, 1], r[:, 2] = image * (s * per + ar(per)), image
        empty.write(data, r, d[s * cap:(s + 1) * cap], dc[s], wparts, wsum, 1 + s * per, TS, out_capacity=per * entry)
    ctx.check()
    assert int(wsum[0].item()) == per
    empty.close()
    p = Walk(torch, ctx, segments, d, dc, cap, 0, nseg, per)
    p.walk(ctx)
    assert int(p.n_entries.item()) == n
    table = ramcrc.ReplayTable(ctx, 2 * n, 1)
    table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work, key_hash=None)
    ctx.check()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    order = torch.randperm(n, device="cuda", generator=g)
    keys = keys[order]
    # every key present; the versions are the write's, 1 + the object's index
    run_shapes(args, np, torch, ramcrc, segments, ctx, table, keys, key_len, {"all_present": z(n, torch.int64)},
               ("all_present",), "keys64",
               dict(value_len=value_len, nseg=nseg, batches=1, segment_bytes=cap, keys=n),
               lambda q: 1 + int(order[q].item()))
    table.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseg", type=int, default=512)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--values", type=lambda s: [int(v) for v in s.split(",") if v], default=[64, 1024, 4096])
    ap.add_argument("--long-keys", type=int, default=1 << 22, help="64-byte keys of the keys64 line; 0: skip it")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=15, help="timed rounds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_table_remove"))
    ap.add_argument("--time-limit", type=int, default=240, help="seconds per line")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        if args.child == "keys64":
            measure_long_keys(args)
        else:
            measure(args, int(args.child))
        return 0
    lines = [str(v) for v in args.values] + (["keys64"] if args.long_keys else [])
    for line in lines:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", line] + sys.argv[1:]
        try:
            rc = subprocess.run(cmd, timeout=args.time_limit).returncode
        except subprocess.TimeoutExpired:
            print("replay_table_remove_bench: a GPU step exceeded its time limit", file=sys.stderr)
            return 124
        if rc:
            return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
