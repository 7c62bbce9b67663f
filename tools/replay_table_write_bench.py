#!/usr/bin/env python3
"""Time a multi-write against the replay table
(ramcrc_replay_table_write_device) beside its parts: the lookup of the same
keys, a device-to-device copy of exactly the output's bytes, and
ramcrc_assemble_objects_device over the written objects in place.

    python tools/replay_table_write_bench.py [--nseg 512] [--batches 8]
                                             [--values 64,1024,4096]
                                             [--out profiles/replay_table_write]

The table is replay_table_read_bench.py's: RecoverSegmentBenchmark-shaped
8 MiB segments built on the device (fill_objects: table 0, 8-byte counter
keys), the first entry of every segment retyped to a SEGHEADER, walked as
--batches batches and added batch by batch.  fill_objects writes version 0,
which a write takes for VERSION_NONEXISTENT, so every object's version is set
to 1 before the add (the walk and the add read no object checksum).

The requests are one-key objects with 8-byte keys and --values value bytes,
the keys of the table in a shuffled order.  Their number is the table's keys
or, if that is fewer, what keeps the output below 4 GiB when every request
writes an object and a tombstone (out_capacity is 32 bits); the JSON says
which.  Three shapes: `all_present` (table 0: object plus tombstone),
`none_present` (the same keys under table 1: the object alone, every version
allocated) and `half` (alternating).  In one round every shape is timed four
ways, each bracketed by device events: the write (hashes computed in the call,
no rules, d_refs, d_old and d_batch_segment_id NULL); the lookup of the same
keys in the same buffer (hashes computed, with counts); a copy of the
output's out_bytes (torch's copy_ of uint8 tensors, which issues
hipMemcpyAsync); and assemble_objects over the written objects where they lie.
The yardstick of a write is lookup + copy + stamp of the same round; the ratio
write / (lookup + copy + stamp) is taken round by round, and the medians are
over --calls rounds after --warmup warm-up rounds.  Every timed write's summary
is checked, and once per shape a write with d_refs checks 256 sampled requests:
entry headers, version, table id, data bytes, the object's checksum and the
tombstone's against the host CRC.  The certificate is not walked here (one
4 GiB segment is one serial walk); the tests do that.  One JSON file per value
size, and one summary line each on stdout.

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
SHAPES = ("all_present", "none_present", "half")
TS = 0x5EC0D5A7


def measure(args, value_len):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import numpy as np
    import torch
    from ramcloud_amd import build, ramcrc, segments
    from replay_table_bench import Walk

    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("replay_table_write_bench: no GPU (no fallback)")
    ctx = ramcrc.Context(0)
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
    n_keys = keys.shape[0]
    assert n_keys == nseg * (per - 1), (n_keys, nseg, per)

    image = 1 + 2 + 8 + value_len            # key count, one cumulative length, the key, the value
    olen, tlen = 24 + image, 32 + 8
    lb = lambda k: 1 if k < 256 else 2 if k < 65536 else 3
    obj_entry, tomb_entry = 1 + lb(olen) + olen, 1 + lb(tlen) + tlen
    fit = ((1 << 32) - 1) // (obj_entry + tomb_entry)
    n = min(n_keys, fit)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    keys = keys[torch.randperm(n_keys, device="cuda", generator=g)[:n]]
    data = torch.empty((n, image), dtype=torch.uint8, device="cuda")
    data.random_(0, 256)
    data[:, 0], data[:, 1], data[:, 2] = 1, 8, 0
    data[:, 3:11] = keys
    data = data.reshape(-1)
    table_of = {"all_present": z(n, torch.int64), "none_present": torch.ones(n, dtype=torch.int64, device="cuda"),
                "half": ar(n) % 2}
    reqs, queries = {}, {}
    for name, tid in table_of.items():
        r = z((n, 3), torch.int64)
        r[:, 0], r[:, 1], r[:, 2] = tid, image * ar(n), image
        q = r.clone()
        q[:, 1] += 3
        q[:, 2] = 8
        reqs[name], queries[name] = r, q
    present = {name: int((tid == 0).sum()) for name, tid in table_of.items()}
    out_bytes = {name: n * obj_entry + present[name] * tomb_entry for name in SHAPES}
    room = max(out_bytes.values())
    assert room < 1 << 32
    out = torch.empty(room, dtype=torch.uint8, device="cuda")
    copy_dst = torch.empty(room, dtype=torch.uint8, device="cuda")
    cert, summary = z(2, torch.int32), z(16, torch.int64)
    wparts = z(3 * n, torch.int32)
    refs = z((n, 2), torch.int32)
    results, counts = z((n, 8), torch.int32), z(5, torch.int64)
    obj_len = torch.full((n,), olen, dtype=torch.int64, device="cuda")
    slots = 64
    while slots < 2 * n:
        slots *= 2
    ctx.reserve(32 + 12 * ((n + 255) // 256), max(8 * n + 2 * slots, max(p.ecap for p in parts)))
    table = ramcrc.ReplayTable(ctx, nseg * per, nb)
    for p in parts:
        table.add(p.d, cap, p.nseg, p.status, p.entries, p.n_entries, p.work, key_hash=None)
    ctx.check()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    nv = 1 << 40

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def want_summary(name):
        p = present[name]
        return dict(dict.fromkeys(segments.WRITE_SUMMARY_DTYPE.names, 0), ok=n, tombstones=p, allocated=n - p,
                    next_version=nv + n - p, out_bytes=out_bytes[name], value_bytes=n * value_len,
                    key_bytes=n * 11, object_bytes=n * olen, tombstone_bytes=p * tlen)

    def got_summary():
        s = summary.cpu().numpy().view(segments.WRITE_SUMMARY_DTYPE)[0]
        return {k: int(s[k]) for k in segments.WRITE_SUMMARY_DTYPE.names}

    def write(name, with_refs=False):
        table.write(data, reqs[name], out, cert, wparts, summary, nv, TS, refs=refs if with_refs else None,
                    out_capacity=out_bytes[name])

    sample = torch.randint(0, n, (256,), device="cuda", generator=g)
    obj_off = {}

    def check(name):
        """256 sampled requests against the host CRC; and where the objects lie."""
        write(name, True)
        assert got_summary() == want_summary(name), got_summary()
        r = refs.cpu().numpy().view(np.uint32)
        obj_off[name] = (refs[:, 0].long() & 0xFFFFFFFF) + 1 + lb(olen)
        pp = wparts.cpu().numpy().view(np.uint8).reshape(n, 12)
        for q in sample.tolist():
            at, tat = int(r[q, 0]), int(r[q, 1])
            o = out[at:at + obj_entry].cpu().numpy().tobytes()
            pay = o[1 + lb(olen):]
            tid = int(table_of[name][q].item())
            status, version = int.from_bytes(pp[q, :4].tobytes(), "little"), int.from_bytes(pp[q, 4:].tobytes(), "little")
            assert o[0] == segments.LOG_ENTRY_TYPE_OBJ | ((lb(olen) - 1) << 6), q
            assert int.from_bytes(o[1:1 + lb(olen)], "little") == olen and status == 0, q
            assert pay[4:8] == TS.to_bytes(4, "little") and pay[8:16] == version.to_bytes(8, "little"), q
            assert pay[16:24] == tid.to_bytes(8, "little"), q
            assert pay[24:] == data[q * image:(q + 1) * image].cpu().numpy().tobytes(), q
            assert int.from_bytes(pay[:4], "little") == ramcrc.crc32c(pay[4:]), q
            if tid == 0:
                t = out[tat:tat + tomb_entry].cpu().numpy().tobytes()
                assert version == 2 and t[0] == segments.LOG_ENTRY_TYPE_OBJTOMB and t[1] == tlen, q
                tp = t[2:]
                assert tp[:8] == bytes(8) and tp[16:24] == (1).to_bytes(8, "little") and tp[32:] == pay[27:35], q
                assert int.from_bytes(tp[28:32], "little") == ramcrc.crc32c(tp[:28] + tp[32:]), q
            else:
                assert tat == 0xFFFFFFFF and version >= nv, q

    def one_round(name):
        t_write = timed(lambda: write(name))
        assert got_summary() == want_summary(name), got_summary()
        t_look = timed(lambda: table.lookup(data, queries[name], results, counts=counts))
        ob = out_bytes[name]
        t_copy = timed(lambda: copy_dst[:ob].copy_(out[:ob]))
        t_stamp = timed(lambda: ctx.assemble_objects(out, obj_off[name], obj_len))
        return t_write, t_look, t_copy, t_stamp

    for name in SHAPES:
        check(name)
    ctx.check()
    for _ in range(args.warmup):
        for name in SHAPES:
            one_round(name)
    ctx.check()
    whats = ("write", "lookup", "copy", "stamp")
    ms = {f"{name}_{what}": [] for name in SHAPES for what in whats}
    for _ in range(args.calls):   # alternate, so that none has the quieter part of the run
        for name in SHAPES:
            for what, t in zip(whats, one_round(name)):
                ms[f"{name}_{what}"].append(t)
    ctx.check()
    mmm = lambda v: [round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)]
    ratio = {name: mmm([w / (lk + c + s) for w, lk, c, s in zip(*(ms[f"{name}_{x}"] for x in whats))])
             for name in SHAPES}
    r = {"value_len": value_len, "nseg": nseg, "batches": nb, "segment_bytes": cap, "keys": n_keys, "requests": n,
         "requests_limited_by": "the table's keys" if n == n_keys else "an output below 4 GiB",
         "out_bytes": out_bytes, "calls_timed": args.calls, "warmup": args.warmup,
         "device": torch.cuda.get_device_name(0), "build": ramcrc.lib().ramcrc_build_info().decode(),
         "ms_median_min_max": {k: mmm(v) for k, v in ms.items()},
         "out_gb_per_s_median": {name: round(out_bytes[name] / float(np.median(ms[name + "_write"])) / 1e6, 1)
                                 for name in SHAPES},
         # per round: the write over the lookup of the same keys, the copy of the output and the stamp
         "ratio_write_over_lookup_plus_copy_plus_stamp_median_min_max": ratio}
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, f"write_{nseg}x8MiB_b{nb}_v{value_len}.json"), "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in r.items())
                + "\n}\n")   # one key per line
    print(json.dumps({"replay_table_write": dict(value_len=value_len, requests=n, ratio=ratio,
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_table_write"))
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
            print("replay_table_write_bench: a GPU step exceeded its time limit", file=sys.stderr)
            return 124
        if rc:
            return rc   # nothing more is started on the GPU after a failure
    return 0


if __name__ == "__main__":
    sys.exit(main())
